"""GPU: a read file that is ONE gzip member (gzip, pigz, a basecaller's output) indexed on the device through the windowed
speculative inflater, and the second pass - the reads' bases cut out of the text by the gather kernel
(rala_hip_slice_sequences) - for plain, BGZF and gzip files.  The verdict is the host readers' (the shim of
tests/test_sequences_cpu.py); the index of x.gz must be the index of x field for field.  Markers are 0x8000 | k: an
off-by-one in the carry or in the windows' rebased offsets shows as wrong bases or as flag 8, and both are looked at."""
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

import test_sequences_cpu as host

pytestmark = pytest.mark.gpu

HALO = 4096


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    return host.synthetic_reads(tmp=tmp_path_factory.mktemp("synth"))


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=9):
    """one gzip member around zlib's raw deflate at `level`"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    body = c.compress(text) + c.flush()
    return b"\x1f\x8b\x08\x00" + b"\x00" * 4 + b"\x00\xff" + body + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


COMPRESSIONS = {"zlib1": lambda t: member(t, 1), "zlib6": lambda t: member(t, 6), "zlib9": lambda t: member(t, 9), "gzip": gzip.compress}


def fnv_many(bases, base_off):
    """host.fnv of every read of a packed array, all reads side by side"""
    starts, lens = base_off[:-1].astype(np.int64), np.diff(base_off.astype(np.int64))
    h = np.full(len(lens), 0xcbf29ce484222325, dtype=np.uint64)
    prime = np.uint64(0x100000001b3)
    for j in range(int(lens.max()) if len(lens) else 0):
        m = np.nonzero(lens > j)[0]
        h[m] = (h[m] ^ bases[starts[m] + j].astype(np.uint64)) * prime
    return h


def index(ctx, path, fastq, window=0, on=1, chunk=0):
    ctx.set_option("gzip_on_device", on)
    ctx.set_option("gzip_chunk_bytes", chunk)
    ctx.set_option("debug_sequence_window", window)
    return ctx.index_sequences(path, fastq)


def sliced(ctx, path, ix, wanted):
    """rala_hip_slice_sequences -> (hashes, base counts) of the wanted reads"""
    wanted = np.asarray(wanted, dtype=np.uint64)
    irregular, bases, base_off = ctx.slice_sequences(path, wanted, ix["length"])
    assert irregular == 0, "the slicer refused with %d" % irregular
    info = ctx.sequence_slice_info()
    assert info["bases"] == int(base_off[-1])
    return fnv_many(bases, base_off), np.diff(base_off.astype(np.int64))


def same_index(a, b):
    assert a["names"] == b["names"]
    for f in ("name_off", "length", "data_off", "data_span"):
        assert a[f].tolist() == b[f].tolist(), f


def same_as_host(ctx, path, fastq, want, window=0, chunk=0):
    """index and bases of a file on the device against the host reader's `want`"""
    irregular, got = index(ctx, path, fastq, window, chunk=chunk)
    assert irregular == 0, "a regular file was handed back with flag %d" % irregular
    assert got["names"] == want["names"]
    assert got["length"].tolist() == want["length"].tolist()
    hashes, counts = sliced(ctx, path, got, np.arange(len(want["names"])))
    assert counts.tolist() == want["length"].tolist()
    assert hashes.tolist() == want["hash"].tolist()
    return got


def shaped(reads, shape):
    fastq = shape.startswith("fastq")
    return fastq, (host.fastq_text(reads) if fastq else host.fasta_text(reads, int(shape[5:])))


def test_fnv_many_is_the_host_hash():
    rng = np.random.default_rng(0)
    bases = rng.integers(0, 256, 1000, dtype=np.uint8)
    off = np.array([0, 0, 1, 500, 1000], dtype=np.uint64)
    assert fnv_many(bases, off).tolist() == [host.fnv(bases[int(a):int(b)].tobytes()) for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("shape", ["fasta1", "fasta60", "fasta80", "fasta0", "fastq"])
def test_equal_to_the_host_reader_and_to_the_plain_files_index(ctx, reads, tmp_path, shape):
    fastq, text = shaped(reads, shape)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    assert len(want["names"]) == len(reads)
    one = same_as_host(ctx, plain, fastq, want)
    for name, compress in COMPRESSIONS.items():
        gz = plain + "." + name + ".gz"
        open(gz, "wb").write(compress(text))
        assert host.host_read(gz, fastq)["hash"].tolist() == want["hash"].tolist()
        same_index(same_as_host(ctx, gz, fastq, want), one)
        t = ctx.gzip_timings()
        assert t["text_bytes"] == len(text) and t["compressed_bytes"] == os.path.getsize(gz)
        assert ctx.sequence_timings()["bytes"] == len(text)


@pytest.mark.parametrize("shape", ["fasta60", "fastq"])
def test_windows(ctx, reads, tmp_path, shape):
    """chunks of 1 KB of compressed bytes and windows of 16 384, 16 385 and 50 001 bytes of text: the one-window index and bases,
    and the getters say that the text did go through several windows of bounded size"""
    fastq, text = shaped(reads, shape)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    for name in ("zlib1", "zlib6", "gzip"):
        gz = plain + "." + name + ".gz"
        open(gz, "wb").write(COMPRESSIONS[name](text))
        one = same_as_host(ctx, gz, fastq, want)
        assert ctx.sequence_slice_info()["windows"] == 1
        for window in (16384, 16385, 50_001):
            same_index(same_as_host(ctx, gz, fastq, want, window, chunk=1024), one)
            t, info = ctx.gzip_timings(), ctx.sequence_slice_info()
            print(name, window, t, info)
            assert t["chunks_confirmed"] >= 8
            assert info["windows"] >= 4
            assert info["max_window_text_bytes"] <= max(window, t["max_wave_text_bytes"]) + HALO


def long_read_fasta():
    rng = np.random.default_rng(1)
    big = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 70_000))
    return b">short\nAC\n>long one\n" + b"\n".join(big[i:i + 1000] for i in range(0, len(big), 1000)) + b"\n>tail\nGG\n"


def test_back_references_across_window_edges(ctx, tmp_path):
    """every read repeats the one before: zlib's matches lie close to 20 000 bytes back, so the first chunk of every window is full
    of markers into the carry; a window is one chunk (no smaller than the largest one).  A chunk can only begin where a deflate
    block begins, and zlib closes a block when its symbol buffer is full: 32 767 symbols at memLevel 9, which is ONE block for
    the whole of this text at levels 6 and 9 - one chunk, one window, nothing across an edge.  So the symbol buffer is made
    small (memLevel 2: 255 symbols; 4: 1 023, where level 1 still finds the repeats); the window, and with it the reach of the
    matches, stays 32 768"""
    rng = np.random.default_rng(5)
    read = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20_000)
    parts = []
    for k in range(12):
        read = read.copy()
        read[rng.integers(0, len(read), 40)] = ord("N")          # a few differences: matches are broken up
        parts.append(b">r%d\n" % k + bytes(read) + b"\n")
    text = b"".join(parts)
    plain = str(tmp_path / "rep.fasta")
    open(plain, "wb").write(text)
    want = host.host_read(plain, False)
    one = same_as_host(ctx, plain, False, want)
    for level, mem_level in ((1, 4), (6, 2), (9, 2)):
        gz = plain + ".%d.gz" % level
        blob = member(text, level, mem_level=mem_level)
        assert len(blob) < len(text) // 3                         # (the repeats were found: there are long-distance matches)
        open(gz, "wb").write(blob)
        for window in (1, 30_000):
            same_index(same_as_host(ctx, gz, False, want, window, chunk=1024), one)
            t, info = ctx.gzip_timings(), ctx.sequence_slice_info()
            print(level, window, len(blob), t, info)
            assert t["chunks_confirmed"] >= 1 and info["windows"] >= 2
            assert info["max_window_text_bytes"] <= max(window, t["max_wave_text_bytes"]) + HALO
    # a read longer than a tile and than the window, LF and CR LF (blocks of 255 symbols again: one of 32 767 holds all of it)
    for eol in (b"\n", b"\r\n"):
        text = long_read_fasta().replace(b"\n", eol)
        plain = str(tmp_path / "long.fasta")
        open(plain, "wb").write(text)
        want = host.host_read(plain, False)
        one = same_as_host(ctx, plain, False, want)
        assert one["length"].tolist() == [2, 70_000, 2]
        open(plain + ".gz", "wb").write(member(text, 6, mem_level=2))
        for window in (1001, 1002, 16384):
            same_index(same_as_host(ctx, plain + ".gz", False, want, window, chunk=1024), one)
            t, info = ctx.gzip_timings(), ctx.sequence_slice_info()
            print(len(eol), window, t, info)
            assert info["windows"] >= 2                            # (the long read lies in more than one of them)
            assert info["max_window_text_bytes"] <= max(window, t["max_wave_text_bytes"]) + HALO


AWKWARD = [(n, False, t) for n, t in sorted(host.AWKWARD_FASTA.items())] + [(n, True, t) for n, t in sorted(host.AWKWARD_FASTQ.items())]


@pytest.mark.parametrize("name,fastq,text", AWKWARD, ids=[("fastq-" if q else "fasta-") + n for n, q, _ in AWKWARD])
def test_awkward_but_regular_files(ctx, tmp_path, name, fastq, text):
    """small single-chunk files, dynamic, fixed (Z_FIXED) and stored (level 0) blocks: indexed and sliced as the host reads them"""
    plain = str(tmp_path / ("x.fastq" if fastq else "x.fasta"))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    one = same_as_host(ctx, plain, fastq, want)
    for tag, blob in (("d", gzip.compress(text)), ("f", member(text, 6, zlib.Z_FIXED)), ("s", member(text, 0))):
        gz = plain + "." + tag + ".gz"
        open(gz, "wb").write(blob)
        assert host.host_read(gz, fastq)["hash"].tolist() == want["hash"].tolist()
        same_index(same_as_host(ctx, gz, fastq, want), one)
        same_index(same_as_host(ctx, gz, fastq, want, 3), one)


def check_slicer(ctx, path, fastq, want, windows, members=None):
    n = len(want["names"])
    sets = [np.arange(n), np.zeros(0, dtype=np.int64), np.arange(0, n, 3), np.arange(n - 1, n)]
    irregular, ix = index(ctx, path, fastq)
    assert irregular == 0
    for window in (0,) + tuple(windows):
        ctx.set_option("debug_sequence_window", window)
        for wanted in sets:
            wanted = wanted[wanted >= 0]
            ref = host.slice_reads(path, ix, wanted, members)
            assert ref is not None
            hashes, counts = sliced(ctx, path, ix, wanted)
            assert counts.tolist() == ref[1].tolist() == want["length"][wanted].tolist()
            assert hashes.tolist() == ref[0].tolist()


@pytest.mark.parametrize("name,fastq,text", AWKWARD, ids=[("fastq-" if q else "fasta-") + n for n, q, _ in AWKWARD])
def test_device_slicer_against_the_host_slicer_tiny_files(ctx, tmp_path, name, fastq, text):
    """windows of 1, 2, 3 and 7 bytes: every record start, CR LF pair and read end lies on a window edge"""
    plain = str(tmp_path / ("x.fastq" if fastq else "x.fasta"))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    if not len(want["names"]):
        return
    check_slicer(ctx, plain, fastq, want, (1, 2, 3, 7))
    blob = host.bgzf(text, list(range(1, min(len(text), 120), 2)), eof=True)
    open(plain + ".gz", "wb").write(blob)
    check_slicer(ctx, plain + ".gz", fastq, want, (1, 2, 3, 7), host.bgzf_members(blob))


@pytest.mark.parametrize("shape", ["fasta1", "fasta60", "fasta0", "fasta80crlf", "fastq", "fastqcrlf"])
def test_device_slicer_against_the_host_slicer_synthetic(ctx, reads, tmp_path, shape):
    fastq = shape.startswith("fastq")
    eol = b"\r\n" if shape.endswith("crlf") else b"\n"
    text = host.fastq_text(reads, eol) if fastq else host.fasta_text(reads, int(shape[5:].replace("crlf", "")), eol)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    check_slicer(ctx, plain, fastq, want, (1001, 1021, 16385))
    blob = host.bgzf(text, list(range(65280, len(text), 65280)))
    open(plain + ".gz", "wb").write(blob)
    check_slicer(ctx, plain + ".gz", fastq, want, (1001, 1021, 16385), host.bgzf_members(blob))


def test_many_tiny_reads_in_one_tile(ctx, tmp_path):
    """thousands of reads of a few bases: more wanted reads in a tile than the gather kernel keeps runs for"""
    rng = np.random.default_rng(9)
    recs = [b">r%d\n%s\n" % (k, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(0, 6))))) for k in range(6000)]
    text = b"".join(recs)
    plain = str(tmp_path / "tiny.fasta")
    open(plain, "wb").write(text)
    want = host.host_read(plain, False)
    check_slicer(ctx, plain, False, want, (16385,))
    open(plain + ".gz", "wb").write(member(text, 6, mem_level=2))      # (blocks of 255 symbols: zlib's usual 32 767 make ONE chunk of it)
    same_as_host(ctx, plain + ".gz", False, want, 20_000, chunk=1024)
    assert ctx.sequence_slice_info()["windows"] >= 2


def _mhap_check(ctx, tmp_path, a_len, b_len):
    """the context's reads through the MHAP tokeniser's length check: -> the read of the first mismatch, or -1"""
    path = str(tmp_path / "probe.mhap")
    open(path, "w").write("1 2 0.1 10 0 0 50 %d 0 0 50 %d\n" % (a_len, b_len))
    bad, irregular = ctypes.c_int64(0), ctypes.c_int(0)
    f = ctx.L.rala_hip_set_overlaps_from_mhap
    f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    ctx.set_option("gzip_on_device", 0)
    assert f(ctx.h, path.encode(), 1, 2, ctypes.byref(bad), ctypes.byref(irregular)) == 0 and irregular.value == 0
    return bad.value


def test_refusals_leave_the_context_as_it_was(ctx, tmp_path):
    fasta = b"".join(b">r%d\n%s\n" % (k, b"ACGTTGCA" * (50 + k % 7)) for k in range(3000))
    good = member(fasta, 6, mem_level=2)                           # (blocks of 255 symbols: several chunks, so several windows)
    body = bytearray(good)
    body[len(good) // 2] ^= 0x10
    crc, isize = bytearray(good), bytearray(good)
    crc[-8] ^= 1
    isize[-4] ^= 1
    multi_line = b"@a\nAC\nGT\n+\nII\nII\n@b\nGG\n+\nII\n"
    cases = [
        ("flipped.fasta.gz", bytes(body), 8, 1),
        ("bad_crc.fasta.gz", bytes(crc), 8, 1),
        ("bad_isize.fasta.gz", bytes(isize), 8, 1),
        ("cut.fasta.gz", good[:len(good) * 2 // 3], 8, 1),
        ("two_members.fasta.gz", good + good, 8, 1),
        ("switch_off.fasta.gz", good, 8, 0),
        ("multi_line.fastq.gz", gzip.compress(multi_line), 1, 1),
    ]
    before = str(tmp_path / "before.fasta")
    open(before, "wb").write(b">x\n" + b"A" * 100 + b"\n>y\n" + b"C" * 200 + b"\n")
    for name, data, flag, on in cases:
        irregular, got = index(ctx, before, False)
        assert irregular == 0 and got["length"].tolist() == [100, 200]
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        for window, chunk in ((0, 0), (20_000, 1024)):
            ctx.set_option("gzip_on_device", on)
            ctx.set_option("gzip_chunk_bytes", chunk)
            ctx.set_option("debug_sequence_window", window)
            n, nb, irr = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(0)
            rc = ctx.L.rala_hip_index_sequences(ctx.h, path.encode(), int(".fastq" in name), 3, ctypes.byref(n), ctypes.byref(nb), ctypes.byref(irr))
            assert rc == 0 and irr.value == flag and n.value == 0 and nb.value == 0, (name, rc, irr.value)
            # no index to fetch or to slice with, and the reads are still those of the file before
            assert ctx.L.rala_hip_get_sequence_index(ctx.h, None, None, None, None, None, None) != 0
            assert ctx.slice_sequences(path, [0], np.array([100, 200]))[0] != 0
            assert _mhap_check(ctx, tmp_path, 100, 200) == -1, name
            assert _mhap_check(ctx, tmp_path, 100, 201) == 1, name
    # the file changes between the index and the slice: another size; the same size, other content
    path = str(tmp_path / "changing.fasta.gz")
    open(path, "wb").write(good)
    want = host.host_read(path, False)
    for window, chunk in ((0, 0), (20_000, 1024)):
        open(path, "wb").write(good)
        ix = same_as_host(ctx, path, False, want, window, chunk)
        assert window == 0 or ctx.sequence_slice_info()["windows"] >= 2
        open(path, "wb").write(good + b"\x00")
        assert ctx.slice_sequences(path, np.arange(len(want["names"])), ix["length"])[0] != 0
        mid = bytearray(good)
        mid[len(good) // 2] ^= 0x10
        open(path, "wb").write(bytes(mid))
        assert ctx.slice_sequences(path, np.arange(len(want["names"])), ix["length"])[0] != 0
        open(path, "wb").write(good)
        hashes, _ = sliced(ctx, path, ix, np.arange(len(want["names"])))
        assert hashes.tolist() == want["hash"].tolist()
    # the same size, other content, and a valid file of its own: stored blocks (the compressed size is the text's plus a constant)
    stored, other = member(fasta, 0), member(fasta.replace(b"ACGTTGCA", b"ACGTTGCT"), 0)
    assert len(stored) == len(other) and stored != other
    open(path, "wb").write(stored)
    ix = same_as_host(ctx, path, False, want)
    open(path, "wb").write(other)
    assert ctx.slice_sequences(path, np.arange(len(want["names"])), ix["length"])[0] != 0
    open(path, "wb").write(other[:-8] + stored[-8:])               # ... under the trailer the index saw
    assert ctx.slice_sequences(path, np.arange(len(want["names"])), ix["length"])[0] != 0
    open(path, "wb").write(stored)
    assert sliced(ctx, path, ix, np.arange(len(want["names"])))[0].tolist() == want["hash"].tolist()
    # with no index at all
    assert index(ctx, str(tmp_path / "two_members.fasta.gz"), False)[0] == 8
    assert ctx.slice_sequences(path, [0], np.array([1]))[0] != 0


def _cli(exe, args, switches):
    env = dict(os.environ, RALA_DEVICE_SEQUENCES=switches, RALA_DEVICE_GZIP=switches, RALA_HIP_TRACE="1")
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    return r.returncode, r.stdout, r.stderr.decode()


def test_cli_with_both_switches_on_and_off(tmp_path):
    """rala reads.fastq.gz ovl.paf, the read file one gzip member: the same contigs with the device index and slicer as with the
    host reader, and the trace says which of them ran"""
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    lines = open(fa, "rb").read().split(b"\n")
    pairs = [(lines[2 * i][1:], lines[2 * i + 1]) for i in range(ds.n_reads)]
    fq = str(tmp_path / "reads.fastq.gz")
    open(fq, "wb").write(gzip.compress(host.fastq_text(pairs), 6))
    rc, out_on, err_on = _cli(exe, [fq, paf], "1")
    assert rc == 0, err_on[-2000:]
    rc, out_off, err_off = _cli(exe, [fq, paf], "0")
    assert rc == 0, err_off[-2000:]
    assert out_on == out_off and len(out_on) > 1000
    assert "device sequence index" in err_on and "device sequence slice" in err_on and "one gzip member" in err_on
    assert "(flags 0)" in err_on.split("device sequence slice")[1].split("\n")[0]
    assert "device sequence" not in err_off
