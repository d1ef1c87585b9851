"""GPU: single-member gzip overlap files (what gzip, pigz, Python's gzip write) inflated on the device by speculative decoding
(option gzip_on_device; rala_amd/csrc/inflate_kernels.hip: find / count / write / windows / resolve) and tokenised there give
exactly what the plain file gives through the device tokeniser - columns, the first length-check offender, the irregular
verdict - across zlib levels and strategies, flush points, header fields and chunk sizes; refuted block starts change
nothing; a file this cannot prove gives irregular & 8 with nothing set; the graph and the CLI from a .gz file are those
from the text.  A fallback (flag 8) on a good file is a failure in every case here.  The streams here are zlib's compressor's
(and one handmade block); what zlib's inflate takes but its compressor never writes, and what it refuses, is held against
the same kernels in tests/test_gpu_inflate_crafted.py.

Data: Dataset(2000, 150 000) is about 9 MB of PAF; zlib's default strategy at memLevel 8 closes a block every 16 383
symbols, a few tens of KB of text each, so such a file holds a few hundred dynamic blocks and chunks of 4 - 16 KB of
compressed bytes find starts by the dozen (the tests print the counts)."""
import ctypes
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

from deflate_craft import LEN_BASE, LEN_EXTRA, _bits, gz_member
import test_gpu_ingest as gi
import test_ingest_cpu as host

pytestmark = pytest.mark.gpu
FIELDS = host.FIELDS
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}
GZ_KEYS = ("find_us", "decode_us", "resolve_us", "compressed_bytes", "text_bytes", "chunks", "with_candidate", "confirmed", "refuted",
           "max_wave_text")


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=0, flush=zlib.Z_FULL_FLUSH):
    """raw deflate of data, `flushes` flush points of kind `flush` spread over it"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body = b""
    cuts = sorted(set(np.linspace(0, len(data), flushes + 2).astype(int).tolist()))
    for a, b in zip(cuts[:-1], cuts[1:]):
        body += c.compress(data[a:b])
        if b < len(data):
            body += c.flush(flush)
    return body + c.flush()


def write_gz(src, dst, name=None, **kw):
    data = open(src, "rb").read()
    blob = gz_member(deflate(data, **kw), data, name)
    assert gzip.decompress(blob) == data
    open(dst, "wb").write(blob)
    return blob


def _lib():
    L = gi._lib()
    L.hp_text_device_with.restype = ctypes.c_void_p
    L.hp_text_device_with.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32,
                                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    L.hp_paf_device_gzip_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def device(path, names, read_len, mhap=False, threads=4, check_lengths=True, on=True, **options):
    """the file through rala_hip_set_overlaps_from_paf / _mhap with options set (gzip_on_device unless on is False)
    -> (columns or None, irregular flags, first length-check offender, the inflater's counts, rows)"""
    L = _lib()
    if on:
        options = dict(options, gzip_on_device=1)
    keys = (ctypes.c_char_p * max(1, len(options)))(*[k.encode() for k in options])
    values = np.array(list(options.values()) + [0], dtype=np.int64)
    rl = np.ascontiguousarray(read_len, dtype=np.uint32)
    h = L.hp_text_device_with(path.encode(), b"" if mhap else "\n".join(names).encode(), rl.ctypes.data, len(rl), int(check_lengths), threads,
                              int(mhap), ctypes.cast(keys, ctypes.c_void_p), values.ctypes.data, len(options))
    try:
        info, g = np.zeros(6, dtype=np.int64), np.zeros(10, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        L.hp_paf_device_gzip_info(h, g.ctypes.data)
        assert info[0] == 0, info
        gz = dict(zip(GZ_KEYS, (int(x) for x in g)))
        if info[1] or info[2] >= 0:
            return None, int(info[1]), int(info[2]), gz, int(info[3])
        n = int(info[3])
        cols = {f: np.zeros(n, dtype=np.uint32) for f in FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in FIELDS], cols["strand"].ctypes.data)
        return cols, 0, -1, gz, n
    finally:
        L.hp_paf_device_free(h)


def same(got, want):
    assert got is not None and want is not None
    for f in list(FIELDS) + ["strand"]:
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), f


def good(res, want, text_bytes=None):
    cols, irregular, bad, gz, _ = res
    print(gz)
    assert irregular == 0 and bad == -1, (irregular, bad, gz)
    same(cols, want)
    if text_bytes is not None:
        assert gz["text_bytes"] == text_bytes
    return gz


def spread(gz):
    """the stream was decoded by several waves: two chunks besides the first confirmed, no wave wrote more than half the text"""
    assert gz["confirmed"] >= 2, gz
    assert 2 * gz["max_wave_text"] <= gz["text_bytes"], gz


@pytest.mark.parametrize("level,strategy", [(0, "default"), (1, "default"), (6, "default"), (9, "default"), (6, "filtered"),
                                            (6, "huffman"), (6, "rle"), (6, "fixed"), (1, "fixed")])
def test_gzip_paf_and_mhap_equal_the_plain_file(tmp_path, level, strategy):
    ds = Dataset(2000, 150_000, 21 + level)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf, mhap = str(tmp_path / "ovl.paf"), str(tmp_path / "ovl.mhap")
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    want, irregular, bad = gi.device_parse(paf, names, ds.read_len)
    assert irregular == 0 and bad == -1
    want_m, irregular, bad = gi.device_parse_mhap(mhap, ds.read_len)
    assert irregular == 0 and bad == -1
    dynamic = strategy == "default" and level > 0
    variants = [(dict(flushes=0), b"ovl", {}),
                (dict(flushes=3, flush=zlib.Z_FULL_FLUSH), None, dict(gzip_chunk_bytes=4096)),
                (dict(flushes=5, flush=zlib.Z_SYNC_FLUSH), b"a name", dict(gzip_chunk_bytes=16384)),
                (dict(flushes=0), None, dict(gzip_chunk_bytes=5000))]
    for plain, w, is_mhap in ((paf, want, False), (mhap, want_m, True)):
        size = os.path.getsize(plain)
        for kw, name, options in variants:
            write_gz(plain, plain + ".gz", name=name, level=level, strategy=STRATEGIES[strategy], **kw)
            gz = good(device(plain + ".gz", names, ds.read_len, mhap=is_mhap, **options), w, size)
            if dynamic and options:
                spread(gz)


def fixed_block_of_far_matches(total):
    """a non-final block of fixed codes (RFC 1951 3.2.6) that copies `total` bytes from distance 32 768 in matches of at
    most 258, then an empty stored block that brings the stream to a byte boundary"""
    out, put, huff = _bits()
    put(0, 1)
    put(1, 2)
    while total:
        n = min(258, total)
        if total - n in (1, 2):         # (no match is shorter than 3)
            n -= 3
        k = 28 if n == 258 else max(i for i in range(28) if LEN_BASE[i] <= n)
        sym = 257 + k
        if sym < 280:
            huff(sym - 256, 7)
        else:
            huff(0xC0 + sym - 280, 8)
        put(n - LEN_BASE[k], LEN_EXTRA[k])
        huff(29, 5)                     # distances 24 577 - 32 768: 13 extra bits
        put(32768 - 24577, 13)
        total -= n
    huff(0, 7)                          # end of block
    put(0, 1)                           # stored, not final
    put(0, 2)
    while len(out) % 8:
        out.append(0)
    body = bytes(sum(b << k for k, b in enumerate(out[i:i + 8])) for i in range(0, len(out), 8))
    return body + b"\x00\x00\xff\xff"


def test_distance_32768_and_matches_across_chunk_starts(tmp_path):
    """a handmade stream: zlib's blocks, then a block whose matches all lie at distance 32 768 (zlib itself never goes beyond
    32 506) copying whole lines from the text in front, then zlib's blocks again - with chunks of 4 KB the wave that meets
    the far matches started less than 32 768 bytes before them, so they copy bytes it does not know"""
    ds = Dataset(1500, 60_000, 8)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "src.paf")
    ds.write_paf(paf)
    lines = open(paf, "rb").read().splitlines(keepends=True)
    head_lines, k = [], 0
    while sum(map(len, head_lines)) < 200_000:
        head_lines.append(lines[k])
        k += 1
    # the lines that will be copied start 32 768 bytes in front of the head's end: its last line is padded with a tag
    cut, tail = len(head_lines) - 1, 0
    while tail + len(head_lines[cut]) <= 32768 - 6:
        tail += len(head_lines[cut])
        cut -= 1
    head_lines[-1] = head_lines[-1][:-1] + b"\tzz:Z:" + b"x" * (32768 - tail - 6) + b"\n"
    t1 = b"".join(head_lines)
    start = len(t1) - 32768
    assert t1[start - 1:start] == b"\n"
    copied = b"".join(head_lines[cut + 1:cut + 40])
    assert t1[start:start + len(copied)] == copied and len(copied) > 2000
    t3 = b"".join(lines[k:])
    c1 = zlib.compressobj(6, zlib.DEFLATED, -15)
    c3 = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c1.compress(t1) + c1.flush(zlib.Z_FULL_FLUSH) + fixed_block_of_far_matches(len(copied)) + c3.compress(t3) + c3.flush()
    text = t1 + copied + t3
    assert zlib.decompressobj(-15).decompress(body) == text
    plain = str(tmp_path / "ovl.paf")
    open(plain, "wb").write(text)
    open(plain + ".gz", "wb").write(gz_member(body, text))
    want, irregular, bad = gi.device_parse(plain, names, ds.read_len)
    assert irregular == 0 and bad == -1
    for chunk in (4096, 1024, 65536):
        gz = good(device(plain + ".gz", names, ds.read_len, gzip_chunk_bytes=chunk), want, len(text))
        if chunk == 4096:
            spread(gz)
        if chunk == 1024:               # smaller than a block: most chunks hold no start, several in a row
            assert gz["with_candidate"] * 2 < gz["chunks"], gz


def test_short_empty_and_unterminated_texts(tmp_path):
    ds = Dataset(500, 20_000, 6)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "all.paf")
    ds.write_paf(paf)
    data = open(paf, "rb").read()
    lines = data.splitlines(keepends=True)
    short = b"".join(lines[:200])
    assert 1000 < len(short) < 32768
    cases = {"short": short, "empty": b"", "one_line": lines[0], "no_newline": data[:-1], "short_no_newline": short[:-1]}
    for name, text in cases.items():
        plain = str(tmp_path / (name + ".paf"))
        open(plain, "wb").write(text)
        want, irregular, bad = gi.device_parse(plain, names, ds.read_len)
        assert irregular == 0 and bad == -1
        for options in ({}, dict(gzip_chunk_bytes=1024)):
            write_gz(plain, plain + ".gz", level=6)
            good(device(plain + ".gz", names, ds.read_len, **options), want, len(text))


@pytest.mark.parametrize("every", [2, 3])
def test_refuted_starts_change_nothing(tmp_path, every):
    ds = Dataset(2000, 150_000, 5)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    want, _, _ = gi.device_parse(paf, names, ds.read_len)
    write_gz(paf, paf + ".gz", level=6)
    for chunk in (4096, 16384):
        gz = good(device(paf + ".gz", names, ds.read_len, gzip_chunk_bytes=chunk, debug_gzip_false_sync=every), want, os.path.getsize(paf))
        assert gz["refuted"] > 0, gz
        spread(gz)


def test_broken_files_are_irregular_and_the_option_defaults_to_off(tmp_path):
    ds = Dataset(1000, 60_000, 2)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    text = open(paf, "rb").read()
    good_blob = write_gz(paf, paf + ".gz", level=6)
    want, _, _ = gi.device_parse(paf, names, ds.read_len)
    good(device(paf + ".gz", names, ds.read_len, gzip_chunk_bytes=8192), want, len(text))
    # the option's default: a plain gzip file is the host reader's, as before
    res = device(paf + ".gz", names, ds.read_len, on=False)
    assert res[0] is None and res[1] & 8 and res[4] == 0 and res[3]["chunks"] == 0
    cases = {}
    b = bytearray(good_blob)
    b[len(b) // 2] ^= 0x55
    cases["flipped"] = bytes(b)
    b = bytearray(good_blob)
    b[-8] ^= 1
    cases["crc"] = bytes(b)
    for delta in (-1, 1):
        b = bytearray(good_blob)
        struct.pack_into("<I", b, len(b) - 4, (len(text) + delta) & 0xFFFFFFFF)
        cases["isize%+d" % delta] = bytes(b)
    cases["cut_in_block"] = good_blob[:len(good_blob) // 3]
    cases["cut_in_trailer"] = good_blob[:-3]
    cases["trailing"] = good_blob + b"trailing bytes\n"
    cases["two_members"] = good_blob + good_blob
    cases["reserved_flag"] = good_blob[:3] + b"\x20" + good_blob[4:]
    for name, data in cases.items():
        path = str(tmp_path / (name + ".paf.gz"))
        open(path, "wb").write(data)
        for chunk in (8192, 1 << 20):
            res = device(path, names, ds.read_len, gzip_chunk_bytes=chunk)
            assert res[0] is None and res[1] & 8 and res[2] == -1 and res[4] == 0, (name, chunk, res[1:])


def test_length_check_first_offender_and_tiny_windows(tmp_path):
    ds = Dataset(2000, 100_000, 9)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    write_gz(paf, paf + ".gz", level=6)
    want, _, _ = gi.device_parse(paf, names, ds.read_len)
    for window in (1 << 20, 37_000):
        good(device(paf + ".gz", names, ds.read_len, threads=3, gzip_chunk_bytes=16384, ingest_window_bytes=window), want)
    lens = np.array(ds.read_len, dtype=np.uint32)
    rows = np.where(ds.overlaps.a_id[len(ds.overlaps.a_id) // 3:] != 0)[0]
    victim = int(ds.overlaps.b_id[len(ds.overlaps.a_id) // 3 + rows[0]])
    lens[victim] += 1
    for window in (0, 50_000):
        for check in (True, False):
            w = gi.device_parse(paf, names, lens, check_lengths=check)
            got = device(paf + ".gz", names, lens, check_lengths=check, ingest_window_bytes=window)
            assert got[1:3] == w[1:]
            if check:
                assert w[2] >= 0 and got[0] is None
            else:
                same(got[0], w[0])


def test_a_call_that_gives_up_in_a_window_leaves_the_context_usable(tmp_path):
    """a gzip PAF with check_lengths on, a tiny window and the first offender in the second of three windows is refused; the
    context stays usable: a plain file ingested on it afterwards gives the host reader's columns"""
    ds = Dataset(500, 20_000, 6)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    lines = open(paf, "rb").read().splitlines(keepends=True)[:600]
    assert len(lines) >= 300
    good_paf, bad_paf = str(tmp_path / "good.paf"), str(tmp_path / "bad.paf")
    open(good_paf, "wb").write(b"".join(lines))
    window = sum(map(len, lines)) // 3 + 1
    k = next(i for i in range(len(lines)) if sum(map(len, lines[:i])) >= window + 100)
    assert sum(map(len, lines[:k + 1])) < 2 * window
    f = lines[k].split(b"\t")
    f[1] = b"%d" % (int(f[1]) + 1)                # (the query's length is no longer its read's)
    open(bad_paf, "wb").write(b"".join(lines[:k] + [b"\t".join(f)] + lines[k + 1:]))
    write_gz(bad_paf, bad_paf + ".gz", level=6)
    want_bad = gi.device_parse(bad_paf, names, ds.read_len)
    assert want_bad[0] is None and want_bad[2] >= 0
    want, e0 = host.parse(good_paf, names, ds.read_len, 2, True)
    assert e0 == -1
    L = _lib()
    L.hp_text_device_after.restype = ctypes.c_void_p
    L.hp_text_device_after.argtypes = [ctypes.c_char_p] + list(L.hp_text_device_with.argtypes)
    L.hp_paf_device_before.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    options = dict(gzip_on_device=1, gzip_chunk_bytes=4096, ingest_window_bytes=window)
    keys = (ctypes.c_char_p * len(options))(*[o.encode() for o in options])
    values = np.array(list(options.values()), dtype=np.int64)
    rl = np.ascontiguousarray(ds.read_len, dtype=np.uint32)
    h = L.hp_text_device_after((bad_paf + ".gz").encode(), good_paf.encode(), "\n".join(names).encode(), rl.ctypes.data, len(rl), 1, 3, 0,
                               ctypes.cast(keys, ctypes.c_void_p), values.ctypes.data, len(options))
    try:
        info, before, g = np.zeros(6, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(10, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        L.hp_paf_device_before(h, before.ctypes.data)
        L.hp_paf_device_gzip_info(h, g.ctypes.data)
        assert info[0] == 0, info
        assert (int(before[0]), int(before[1])) == want_bad[1:], before
        assert info[1] == 0 and info[2] == -1 and info[3] == len(lines), info
        assert g[5] == 0, g                     # (the second file met no inflater)
        cols = {f: np.zeros(len(lines), dtype=np.uint32) for f in FIELDS}
        cols["strand"] = np.zeros(len(lines), dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in FIELDS], cols["strand"].ctypes.data)
        same(cols, want)
    finally:
        L.hp_paf_device_free(h)


def _mhap_graph(path, read_len, options=()):
    ctx = hip.Context(0)
    try:
        for k, v in options:
            ctx.set_option(k, v)
        ctx.set_reads(read_len)
        bad, irregular = ctypes.c_int64(0), ctypes.c_int(0)
        f = ctx.L.rala_hip_set_overlaps_from_mhap
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        assert f(ctx.h, path.encode(), 1, 8, ctypes.byref(bad), ctypes.byref(irregular)) == 0
        assert bad.value == -1 and irregular.value == 0
        tm = hip.GzipTimings()
        assert ctx.L.rala_hip_get_gzip_timings(ctx.h, ctypes.byref(tm)) == 0
        n = ctypes.c_uint64(0)
        assert ctx.L.rala_hip_get_overlap_columns(ctx.h, ctypes.byref(n), None, None) == 0
        ctx.n_overlaps = n.value
        ctx.initialize()
        ctx.construct()
        n_tr = ctx.remove_transitive_edges()
        return (n_tr, ctx.graph(), ctx.piles(), ctx.valid(), ctx.pile_row_digests()), tm.as_dict()
    finally:
        ctx.close()


def test_graph_from_gzip_equals_graph_from_text(tmp_path):
    ds = Dataset(20_000, 2_000_000, 3)
    paf, mhap = str(tmp_path / "ovl.paf"), str(tmp_path / "ovl.mhap")
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    os.remove(paf)
    subprocess.run(["gzip", "-6", "-k", mhap], check=True)
    a, tm = _mhap_graph(mhap, ds.read_len)
    assert tm["chunks"] == 0
    b, tm = _mhap_graph(mhap + ".gz", ds.read_len, [("gzip_on_device", 1)])
    print(tm)
    assert tm["text_bytes"] == os.path.getsize(mhap) and tm["chunks_confirmed"] >= 2
    assert a[0] == b[0] and a[0] > 0
    for x, y in zip(a[1:], b[1:]):
        if isinstance(x, dict):
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
        elif isinstance(x, (tuple, list)):
            for u, v in zip(x, y):
                assert np.array_equal(np.asarray(u), np.asarray(v))
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y))


def _cli(exe, fa, ovl, env_extra):
    env = dict(os.environ, RALA_HIP_TRACE="1", **env_extra)
    r = subprocess.run([exe, fa, ovl], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    err = r.stderr.decode()
    return r.returncode, r.stdout, [x for x in err.splitlines() if "number of" in x], err


def test_cli_gzip_paf(tmp_path):
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    rc, out, numbers, _ = _cli(exe, fa, paf, {})
    assert rc == 0 and len(out) > 1000
    subprocess.run(["gzip", "-6", "-k", paf], check=True)
    for env, inflated in (({"RALA_DEVICE_GZIP": "1"}, True), ({"RALA_DEVICE_INGEST": "0"}, False), ({"RALA_DEVICE_GZIP": "0"}, False)):
        rc2, out2, numbers2, err = _cli(exe, fa, paf + ".gz", env)
        assert rc2 == 0, err[-2000:]
        assert out2 == out and numbers2 == numbers
        assert ("device inflate: one gzip member" in err) == inflated, err[-2000:]
