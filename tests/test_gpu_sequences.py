"""GPU: the sequence index (rala_hip_index_sequences, rala_amd/csrc/sequence_kernels.hip) gives, for FASTA and four-line FASTQ,
plain and BGZF, the names and lengths of io::read_fasta / io::read_fastq, and offsets with which the second pass's slicer cuts
out exactly the bases those readers hand over.  The verdict for every file is the host readers' (the shim of
tests/test_sequences_cpu.py), never what the file's author meant.  Awkward but regular files must be indexed, not handed back;
windows of any size give the one-window index; irregular files give their flag and leave the context as it was; the command
line gives the same output with the switch on and off."""
import ctypes
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

import test_sequences_cpu as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    return host.synthetic_reads(tmp=tmp_path_factory.mktemp("synth"))


def index(ctx, path, fastq, window=0):
    ctx.set_option("debug_sequence_window", window)
    return ctx.index_sequences(path, fastq)


def same_as_host(ctx, path, fastq, window=0, blob=None):
    """the device's index of the file against the host reader; the bases through the slicer with the device's index"""
    want = host.host_read(path, fastq)
    irregular, got = index(ctx, path, fastq, window)
    assert irregular == 0, "a regular file was handed back with flag %d" % irregular
    assert got["names"] == want["names"]
    assert got["length"].tolist() == want["length"].tolist()
    if len(want["names"]):
        members = host.bgzf_members(blob) if blob is not None else None
        sliced = host.slice_reads(path, got, np.arange(len(want["names"])), members)
        assert sliced is not None
        assert sliced[1].tolist() == want["length"].tolist() and sliced[0].tolist() == want["hash"].tolist()
    return got


def same_index(a, b):
    assert a["names"] == b["names"]
    for f in ("name_off", "length", "data_off", "data_span"):
        assert a[f].tolist() == b[f].tolist(), f


def shaped(reads, shape):
    fastq = shape.startswith("fastq")
    return fastq, (host.fastq_text(reads) if fastq else host.fasta_text(reads, int(shape[5:])))


@pytest.mark.parametrize("shape", ["fasta1", "fasta60", "fasta80", "fasta0", "fastq"])
def test_names_lengths_and_bases_equal_the_host_readers(ctx, reads, tmp_path, shape):
    fastq, text = shaped(reads, shape)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    one = same_as_host(ctx, plain, fastq)
    assert len(one["names"]) == len(reads)
    t = ctx.sequence_timings()
    assert t["bytes"] == len(text) and t["lines"] == len(reads)
    # bgzip's shape: members of 65280 bytes of text; and members of every size
    rng = np.random.default_rng(len(text))
    for k, cuts in enumerate((range(65280, len(text), 65280), np.cumsum(rng.integers(1, 60000, 200)).tolist())):
        blob = host.bgzf(text, list(cuts), eof=k == 0)
        gz = plain + ".gz"
        open(gz, "wb").write(blob)
        same_index(same_as_host(ctx, gz, fastq, blob=blob), one)
    # windows over the text, plain and BGZF (members shipped window by window)
    for window in (16384, 16385, 50_001):
        same_index(same_as_host(ctx, plain, fastq, window), one)
    same_index(same_as_host(ctx, gz, fastq, 40_000, blob=blob), one)


def long_read_fasta():
    rng = np.random.default_rng(1)
    big = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 70_000))
    return b">short\nAC\n>long one\n" + b"\n".join(big[i:i + 1000] for i in range(0, len(big), 1000)) + b"\n>tail\nGG\n"


REGULAR = [(n, False, t) for n, t in sorted(host.AWKWARD_FASTA.items())] + [(n, True, t) for n, t in sorted(host.AWKWARD_FASTQ.items())]
REGULAR.append(("name_of_1024_bytes", False, b">" + b"n" * 1024 + b" d\nAC\n>" + b"m" * 1024 + b"\nGT\n"))
REGULAR.append(("long_description", False, b">a " + b"d" * 3000 + b"\nAC\n>b\nGT\n"))


@pytest.mark.parametrize("name,fastq,text", REGULAR, ids=[("fastq-" if q else "fasta-") + n for n, q, _ in REGULAR])
def test_awkward_but_regular_files_in_every_window(ctx, tmp_path, name, fastq, text):
    """each is indexed (never handed back) and equals the host reader; then windows of 1, 2, 3 and 7 bytes - with 1 every
    record start, header end and CR LF pair of the file lies on a window edge - and BGZF members that end at EVERY offset"""
    path = str(tmp_path / ("x.fastq" if fastq else "x.fasta"))
    open(path, "wb").write(text)
    one = same_as_host(ctx, path, fastq)
    windows = (1, 2, 3, 7) if len(text) < 200 else (1021, 1024, 1500)
    for window in windows:
        same_index(same_as_host(ctx, path, fastq, window), one)
    # members of one byte each up to 120 bytes (ends inside names, between CR and LF, behind '>'), empty members among them
    blob = host.bgzf(text, list(range(1, min(len(text), 120))), eof=len(text) % 2 == 0, empty_at=(0, 3, 4))
    gz = path + ".gz"
    open(gz, "wb").write(blob)
    same_index(same_as_host(ctx, gz, fastq, blob=blob), one)
    same_index(same_as_host(ctx, gz, fastq, 5 if len(text) < 200 else 1021, blob=blob), one)


def test_a_read_longer_than_a_tile_and_than_the_window(ctx, tmp_path):
    text = long_read_fasta()
    path = str(tmp_path / "long.fasta")
    open(path, "wb").write(text)
    one = same_as_host(ctx, path, False)
    assert one["length"].tolist() == [2, 70_000, 2] and one["data_span"][1] == 70_070
    for window in (1000, 1001, 16384, 20_000):
        same_index(same_as_host(ctx, path, False, window), one)
    crlf = text.replace(b"\n", b"\r\n")
    open(path, "wb").write(crlf)
    one = same_as_host(ctx, path, False)
    for window in (1001, 1002, 16384):            # CR LF pairs lie 1002 bytes apart: every one is cut by some window
        same_index(same_as_host(ctx, path, False, window), one)
    blob = host.bgzf(crlf, list(range(1001, len(crlf), 1002)))        # members that end between CR and LF
    open(path + ".gz", "wb").write(blob)
    same_index(same_as_host(ctx, path + ".gz", False, blob=blob), one)


def _mhap_check(ctx, tmp_path, a_len, b_len):
    """the context's reads through the MHAP tokeniser's length check: -> the read of the first mismatch, or -1"""
    path = str(tmp_path / "probe.mhap")
    open(path, "w").write("1 2 0.1 10 0 0 50 %d 0 0 50 %d\n" % (a_len, b_len))
    f = ctx.L.rala_hip_set_overlaps_from_mhap
    f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    bad, irregular = ctypes.c_int64(0), ctypes.c_int(0)
    assert f(ctx.h, path.encode(), 1, 2, ctypes.byref(bad), ctypes.byref(irregular)) == 0 and irregular.value == 0
    return bad.value


def irregular_files(tmp_path):
    good = b"@a\nACGT\n+\nIIII\n@b\nGG\n+\nII\n"
    fasta = b">a\nACGT\n>b\nGG\n" * 3000
    blob = host.bgzf(fasta, list(range(20_000, len(fasta), 20_000)))
    cut = blob[:len(blob) // 2]
    crc = bytearray(blob)
    first = struct.unpack_from("<H", blob, 16)[0] + 1
    crc[first - 8] ^= 1                         # the first member's CRC32
    return [
        ("multi_line.fastq", b"@a\nAC\nGT\n+\nII\nII\n@b\nGG\n+\nII\n", 1),
        ("blank_between.fastq", b"@a\nACGT\n+\nIIII\n\n@b\nGG\n+\nII\n", 1),
        ("blank_lines_between.fastq", b"@a\nACGT\n+\nIIII\n\n\n\n\n@b\nGG\n+\nII\n", 1),
        ("short_quality.fastq", b"@a\nACGT\n+\nIII\n@b\nGG\n+\nII\n", 1),
        ("long_quality.fastq", b"@a\nACGT\n+\nIIIII\n@b\nGG\n+\nII\n", 1),
        ("cut_1.fastq", good + b"@c\n", 1),
        ("cut_2.fastq", good + b"@c\nAC\n", 1),
        ("cut_3.fastq", good + b"@c\nAC\n+\n", 1),
        ("no_plus.fastq", b"@a\nACGT\n-\nIIII\n", 1),
        ("long_name.fasta", b">a\nAC\n>" + b"n" * 1025 + b"\nGT\n", 2),
        ("long_name.fastq", b"@" + b"n" * 1025 + b" d\nGT\n+\nII\n", 2),
        ("plain_gzip.fasta.gz", gzip.compress(fasta), 8),
        ("cut_member.fasta.gz", cut, 8),
        ("bad_crc.fasta.gz", bytes(crc), 8),
    ]


def test_irregular_files_give_their_flag_and_set_nothing(ctx, tmp_path):
    before = str(tmp_path / "before.fasta")
    open(before, "wb").write(b">x\n" + b"A" * 100 + b"\n>y\n" + b"C" * 200 + b"\n")
    for name, data, flag in irregular_files(tmp_path):
        irregular, got = index(ctx, before, False)
        assert irregular == 0 and got["length"].tolist() == [100, 200]
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        fastq = ".fastq" in name
        n, nb, irr = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(0)
        rc = ctx.L.rala_hip_index_sequences(ctx.h, path.encode(), int(fastq), 3, ctypes.byref(n), ctypes.byref(nb), ctypes.byref(irr))
        assert rc == 0 and irr.value & flag and n.value == 0 and nb.value == 0, (name, rc, irr.value)
        # no index to fetch, and the reads are still those of the file before: the tokeniser's length check sees 100 and 200
        assert ctx.L.rala_hip_get_sequence_index(ctx.h, None, None, None, None, None, None) != 0
        assert _mhap_check(ctx, tmp_path, 100, 200) == -1, name
        assert _mhap_check(ctx, tmp_path, 100, 201) == 1, name
        if flag == 1:
            # ... in every window too
            ctx.set_option("debug_sequence_window", 3)
            rc = ctx.L.rala_hip_index_sequences(ctx.h, path.encode(), int(fastq), 3, ctypes.byref(n), ctypes.byref(nb), ctypes.byref(irr))
            assert rc == 0 and irr.value & flag, name
            ctx.set_option("debug_sequence_window", 0)


def test_a_fifo_is_not_a_file(ctx, tmp_path):
    path = str(tmp_path / "pipe.fasta")
    os.mkfifo(path)
    fd = os.open(path, os.O_RDWR)          # (so that the library's open does not wait for a writer)
    try:
        n, nb, irr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        rc = ctx.L.rala_hip_index_sequences(ctx.h, path.encode(), 0, 2, ctypes.byref(n), ctypes.byref(nb), ctypes.byref(irr))
        assert hip.ERRORS[rc] == "ENOTAFILE"
    finally:
        os.close(fd)


def _cli(exe, args, mode, trace=True):
    env = dict(os.environ, RALA_DEVICE_SEQUENCES=mode)
    if trace:
        env["RALA_HIP_TRACE"] = "1"
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    return r.returncode, r.stdout, r.stderr.decode()


def test_cli_with_the_switch_on_and_off(tmp_path):
    """plain FASTA and BGZF FASTQ: the contigs, the graph's dumps (rala -d: CSV and JSON - the command line writes no GFA) and the
    trimmed reads of rala -p are byte for byte the same with RALA_DEVICE_SEQUENCES=1 and =0"""
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    lines = open(fa, "rb").read().split(b"\n")
    pairs = [(lines[2 * i][1:], lines[2 * i + 1]) for i in range(ds.n_reads)]
    open(fa, "wb").write(host.fasta_text(pairs, 80))
    fq_text = host.fastq_text(pairs)
    fq = str(tmp_path / "reads.fastq.gz")
    open(fq, "wb").write(host.bgzf(fq_text, list(range(65280, len(fq_text), 65280))))
    results = {}
    for reads_file in (fa, fq):
        for mode in ("1", "0"):
            prefix = str(tmp_path / ("dbg" + mode))
            rc, out, err = _cli(exe, ["-d", prefix, reads_file, paf], mode)
            assert rc == 0, err[-2000:]
            assert ("device sequence index" in err) == (mode == "1"), err[-2000:]
            rc, nodes, err = _cli(exe, ["-p", reads_file, paf], mode, trace=False)
            assert rc == 0, err[-2000:]
            results[(reads_file, mode)] = (out, open(prefix + ".csv", "rb").read(), open(prefix + ".json", "rb").read(), nodes)
        assert results[(reads_file, "1")] == results[(reads_file, "0")]
        assert len(results[(reads_file, "1")][0]) > 1000 and len(results[(reads_file, "1")][3]) > 1000
    assert results[(fa, "1")] == results[(fq, "1")]
