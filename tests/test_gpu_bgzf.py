"""GPU: BGZF overlap files inflated on the device (rala_amd/csrc/inflate_kernels.hip) and tokenised there give exactly what the
plain file gives through the device tokeniser - columns, the first length-check offender, the irregular verdict - across zlib
levels and strategies, member sizes, several deflate blocks per member, lines cut at member edges and tiny windows; a broken
or non-BGZF gzip file gives irregular & 8 with nothing set (the caller's host reader then decides); the CLI and the graph
from a BGZF file are those from the plain one."""
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

import test_gpu_ingest as gi
import test_ingest_cpu as host

pytestmark = pytest.mark.gpu
FIELDS = host.FIELDS
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}


def member(data, level=1, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=0):
    """one BGZF member (tests/test_ingest_cpu.py::_write_bgzf's layout); flushes: Z_FULL_FLUSH that many times inside it
    (several deflate blocks, the last ones byte aligned)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body = b""
    cuts = sorted(set(np.linspace(0, len(data), flushes + 2).astype(int).tolist()))
    for a, b in zip(cuts[:-1], cuts[1:]):
        body += c.compress(data[a:b])
        if b < len(data):
            body += c.flush(zlib.Z_FULL_FLUSH)
    body += c.flush()
    total = 18 + len(body) + 8
    assert total <= 65536
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1) +
            body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_bgzf(src, dst, sizes, eof=True, **kw):
    """src's bytes as members of sizes(i) bytes of text each"""
    data = open(src, "rb").read()
    out, i, k = [], 0, 0
    while i < len(data):
        n = sizes(k)
        out.append(member(data[i:i + n], **kw))
        i += n
        k += 1
    if eof:
        out.append(member(b""))
    open(dst, "wb").write(b"".join(out))
    return out


def random_sizes(seed, hi=65536):
    rng = np.random.default_rng(seed)
    return lambda k: int(rng.integers(1, hi + 1))


def same(got, want):
    assert got is not None and want is not None
    for f in list(FIELDS) + ["strand"]:
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), f


def raw_device(path, names, read_len, threads=4, check_lengths=True, mhap=False):
    """-> info of librala_api's device ingest: rc, irregular, length error, rows, ship us, tokenise us"""
    L = gi._lib()
    rl = np.ascontiguousarray(read_len, dtype=np.uint32)
    h = (L.hp_mhap_device(path.encode(), rl.ctypes.data, len(rl), int(check_lengths), threads) if mhap else
         L.hp_paf_device(path.encode(), "\n".join(names).encode(), rl.ctypes.data, len(names), int(check_lengths), threads))
    try:
        info = np.zeros(6, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        return info
    finally:
        L.hp_paf_device_free(h)


@pytest.mark.parametrize("level,strategy", [(0, "default"), (1, "default"), (6, "default"), (9, "default"), (6, "filtered"),
                                            (6, "huffman"), (6, "rle"), (6, "fixed"), (1, "fixed")])
def test_bgzf_paf_and_mhap_equal_the_plain_file(tmp_path, level, strategy):
    ds = Dataset(2000, 150_000, 11 + level)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf, mhap = str(tmp_path / "ovl.paf"), str(tmp_path / "ovl.mhap")
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    want, irregular, bad = gi.device_parse(paf, names, ds.read_len)
    assert irregular == 0 and bad == -1
    want_m, irregular, bad = gi.device_parse_mhap(mhap, ds.read_len)
    assert irregular == 0 and bad == -1
    hi = 65000 if level == 0 else 65536
    for seed, flushes in ((level, 0), (level + 100, 3)):
        kw = dict(level=level, strategy=STRATEGIES[strategy], flushes=flushes)
        write_bgzf(paf, paf + ".gz", random_sizes(seed, hi), eof=seed % 2 == 0, **kw)
        got, irregular, bad = gi.device_parse(paf + ".gz", names, ds.read_len)
        assert irregular == 0 and bad == -1
        same(got, want)
        write_bgzf(mhap, mhap + ".gz", random_sizes(seed + 1, hi), **kw)
        got, irregular, bad = gi.device_parse_mhap(mhap + ".gz", ds.read_len)
        assert irregular == 0 and bad == -1
        same(got, want_m)


def test_full_members_line_cuts_and_tiny_windows(tmp_path, monkeypatch):
    """members of exactly 65536 bytes, of one byte, cuts inside lines and names; windows of 1 MB and 37 KB over the text"""
    ds = Dataset(3000, 300_000, 4)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    want, _, _ = gi.device_parse(paf, names, ds.read_len)
    pattern = [65536, 1, 7, 65536, 30000, 2, 65535]
    write_bgzf(paf, paf + ".gz", lambda k: pattern[k % len(pattern)], level=6)
    got, irregular, bad = gi.device_parse(paf + ".gz", names, ds.read_len)
    assert irregular == 0 and bad == -1
    same(got, want)
    for window in (1 << 20, 37_000):
        monkeypatch.setenv("RALA_INGEST_WINDOW", str(window))
        got, irregular, bad = gi.device_parse(paf + ".gz", names, ds.read_len, 3)
        assert irregular == 0 and bad == -1
        same(got, want)


def test_length_check_first_offender(tmp_path, monkeypatch):
    ds = Dataset(2000, 100_000, 9)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    lens = np.array(ds.read_len, dtype=np.uint32)
    rows = np.where(ds.overlaps.a_id[len(ds.overlaps.a_id) // 3:] != 0)[0]
    victim = int(ds.overlaps.b_id[len(ds.overlaps.a_id) // 3 + rows[0]])
    lens[victim] += 1
    write_bgzf(paf, paf + ".gz", random_sizes(5))
    for window in (None, "50000"):
        if window:
            monkeypatch.setenv("RALA_INGEST_WINDOW", window)
        for check in (True, False):
            want = gi.device_parse(paf, names, lens, check_lengths=check)
            got = gi.device_parse(paf + ".gz", names, lens, check_lengths=check)
            assert got[1:] == want[1:]
            if check:
                assert want[2] >= 0 and got[0] is None
            else:
                same(got[0], want[0])


def test_broken_and_plain_gzip_files_are_irregular(tmp_path):
    ds = Dataset(1000, 60_000, 2)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf = str(tmp_path / "ovl.paf")
    ds.write_paf(paf)
    members = write_bgzf(paf, paf + ".gz", lambda k: 40000)
    good = open(paf + ".gz", "rb").read()
    assert gi.device_parse(paf + ".gz", names, ds.read_len)[1] == 0
    k = len(members) // 2
    at = sum(len(m) for m in members[:k])
    cases = {}
    b = bytearray(good)
    b[at + 18 + len(members[k]) // 3] ^= 0x55
    cases["flipped"] = bytes(b)
    b = bytearray(good)
    b[at + len(members[k]) - 8] ^= 1
    cases["crc"] = bytes(b)
    for delta in (-1, 1):
        b = bytearray(good)
        struct.pack_into("<I", b, at + len(members[k]) - 4, 40000 + delta)
        cases["isize%+d" % delta] = bytes(b)
    cases["cut"] = good[:at + 100]
    cases["cut_trailer"] = good[:len(good) - 28 - 3]
    cases["trailing"] = good + b"trailing bytes\n"
    cases["plain_gzip"] = gzip.compress(open(paf, "rb").read())
    for name, data in cases.items():
        path = str(tmp_path / (name + ".paf.gz"))
        open(path, "wb").write(data)
        info = raw_device(path, names, ds.read_len)
        assert info[0] == 0 and info[1] & 8 and info[3] == 0, (name, info)
        if name == "plain_gzip":
            assert info[4] == 0 and info[5] == 0, info          # nothing shipped: known from the header


def _cli(exe, fa, ovl, mode, trace=False):
    env = dict(os.environ, RALA_DEVICE_INGEST=mode)
    if trace:
        env["RALA_HIP_TRACE"] = "1"
    r = subprocess.run([exe, fa, ovl], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    err = r.stderr.decode()
    return r.returncode, r.stdout, [x for x in err.splitlines() if "number of" in x], err


def test_cli_bgzf_paf_and_mhap(tmp_path):
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf, mhap = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf"), str(tmp_path / "ovl.mhap")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    for plain in (paf, mhap):
        write_bgzf(plain, plain + ".gz", random_sizes(3))
        rc, out, numbers, _ = _cli(exe, fa, plain, "1")
        assert rc == 0 and len(out) > 1000
        for mode in ("1", "0"):
            rc2, out2, numbers2, err = _cli(exe, fa, plain + ".gz", mode, trace=True)
            assert rc2 == 0, err[-2000:]
            assert out2 == out and numbers2 == numbers
            assert ("device inflate" in err) == (mode == "1"), err[-2000:]
    # a corrupted file: the same exit status and error line with the device ingest and without it
    b = bytearray(open(paf + ".gz", "rb").read())
    b[70000] ^= 0xFF
    bad = str(tmp_path / "bad.paf.gz")
    open(bad, "wb").write(bytes(b))
    r1, r0 = _cli(exe, fa, bad, "1"), _cli(exe, fa, bad, "0")
    assert r1[0] == r0[0] != 0
    assert r1[3].strip().splitlines()[-1] == r0[3].strip().splitlines()[-1]


def _mhap_graph(path, read_len):
    """initialize / construct / remove_transitive_edges from an MHAP file ingested on the device, in this process"""
    ctx = hip.Context(0)
    try:
        ctx.set_reads(read_len)
        bad, irregular = ctypes.c_int64(0), ctypes.c_int(0)
        f = ctx.L.rala_hip_set_overlaps_from_mhap
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        assert f(ctx.h, path.encode(), 1, 8, ctypes.byref(bad), ctypes.byref(irregular)) == 0
        assert bad.value == -1 and irregular.value == 0
        n = ctypes.c_uint64(0)
        assert ctx.L.rala_hip_get_overlap_columns(ctx.h, ctypes.byref(n), None, None) == 0
        ctx.n_overlaps = n.value
        ctx.initialize()
        ctx.construct()
        n_tr = ctx.remove_transitive_edges()
        return n_tr, ctx.graph(), ctx.piles(), ctx.valid(), ctx.pile_row_digests()
    finally:
        ctx.close()


def test_graph_from_bgzf_equals_graph_from_text(tmp_path):
    ds = Dataset(20_000, 2_000_000, 3)
    paf, mhap = str(tmp_path / "ovl.paf"), str(tmp_path / "ovl.mhap")
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    os.remove(paf)
    write_bgzf(mhap, mhap + ".gz", lambda k: 65280)
    a = _mhap_graph(mhap, ds.read_len)
    b = _mhap_graph(mhap + ".gz", ds.read_len)
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
