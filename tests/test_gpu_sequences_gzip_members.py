"""GPU: read files that are SEVERAL gzip members (cat fastq_pass/*.fastq.gz > reads.fastq.gz - how most nanopore read sets
arrive) indexed and sliced on the device with the options gzip_on_device and gzip_members, window by window: any number of
member boundaries in a window, a boundary in the bytes the index holds back between two windows, every member proven by its
own CRC32 and ISIZE in both passes.  The verdict is the host readers' (zlib's gzread walks the members) and the plain file's
index; the bases are those io::slice_sequences cuts out of the plain file."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

import test_gpu_sequences_gzip as gs
import test_sequences_cpu as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.set_option("gzip_members", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    return host.synthetic_reads(n_reads=32, genome=20_000, tmp=tmp_path_factory.mktemp("synth"))      # (0.3 MB as FASTA, 0.6 MB as FASTQ)


def members_of(text, cuts, level=6, mem_level=2):
    """text as gzip members that end at `cuts` (blocks of 255 symbols: several chunks per member)"""
    at = [0] + sorted(cuts) + [len(text)]
    return [gs.member(text[a:b], level, mem_level=mem_level) for a, b in zip(at[:-1], at[1:])]


def listed(text, cuts):
    at = [0] + sorted(cuts) + [len(text)]
    return [(a, b - a, zlib.crc32(text[a:b]) & 0xFFFFFFFF) for a, b in zip(at[:-1], at[1:])]


def cut_points(text, fastq, n, where, seed=1):
    """n - 1 cuts: at record starts, in the middle of a line of bases, or in the middle of a header's name"""
    arr = np.frombuffer(text, dtype=np.uint8)
    starts = np.flatnonzero((arr[1:] == (ord("@") if fastq else ord(">"))) & (arr[:-1] == 10)) + 1
    if fastq:                                       # (a quality line may begin with '@': every fourth line start is a record's)
        lines = np.concatenate([[0], np.flatnonzero(arr[:-1] == 10) + 1])
        starts = lines[4::4]
    rng = np.random.default_rng(seed)
    picked = np.sort(rng.choice(starts, n - 1, replace=False))
    if where == "record":
        return picked.tolist()
    if where == "name":
        return (picked + 2).tolist()                # between the first and the second byte of the name
    out = []
    for p in picked.tolist():                       # the middle of the line behind the header
        nl = text.index(b"\n", p)
        end = text.index(b"\n", nl + 1)
        out.append((nl + 1 + end) // 2)
    return out


def check(ctx, path, fastq, want, one, plain, members, window=0, chunk=0, wanted=None):
    ix = gs.same_as_host(ctx, path, fastq, want, window, chunk)
    gs.same_index(ix, one)
    assert ctx.gzip_members() == members
    n = len(want["names"])
    wanted = np.arange(0, n, 3) if wanted is None else wanted
    ref = host.slice_reads(plain, ix, wanted)
    assert ref is not None
    hashes, counts = gs.sliced(ctx, path, ix, wanted)
    assert hashes.tolist() == ref[0].tolist() and counts.tolist() == ref[1].tolist()
    return ix


@pytest.mark.parametrize("where", ["record", "line", "name"])
@pytest.mark.parametrize("n_members", [2, 30])
@pytest.mark.parametrize("shape", ["fasta60", "fastq"])
def test_index_and_bases_equal_the_plain_file_and_the_host_reader(ctx, reads, tmp_path, shape, n_members, where):
    fastq, text = gs.shaped(reads, shape)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    one = gs.same_as_host(ctx, plain, fastq, want)
    cuts = cut_points(text, fastq, n_members, where)
    if where != "record":
        assert any(text[c - 1:c] != b"\n" for c in cuts)
    blob = b"".join(members_of(text, cuts))
    assert gzip.decompress(blob) == text
    gz = plain + ".gz"
    open(gz, "wb").write(blob)
    assert host.host_read(gz, fastq)["hash"].tolist() == want["hash"].tolist()
    members = listed(text, cuts)
    # the default window: all of it in one
    check(ctx, gz, fastq, want, one, plain, members)
    assert ctx.sequence_slice_info()["windows"] == 1 and ctx.gzip_timings()["text_bytes"] == len(text)
    # windows down to one chunk of 1 KB of compressed bytes each
    for window in (50_001, 16384, 1):
        check(ctx, gz, fastq, want, one, plain, members, window, 1024)
        t, info = ctx.gzip_timings(), ctx.sequence_slice_info()
        print(shape, n_members, where, window, t, info)
        assert info["windows"] >= 4 and t["chunks_confirmed"] >= 8
        assert info["max_window_text_bytes"] <= max(window, t["max_wave_text_bytes"]) + gs.HALO


@pytest.mark.parametrize("shape", ["fasta60", "fastq"])
def test_a_member_boundary_inside_the_bytes_held_back_between_windows(ctx, reads, tmp_path, shape):
    """windows of one chunk, and a member of 1500 bytes of text between two large ones: the window that holds it is the 4096 bytes
    held back of the window before and the small member, of which the last 4096 are held back again - the boundary in front of the
    small member lies inside them, the one behind it at their end"""
    fastq, text = gs.shaped(reads, shape)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    want = host.host_read(plain, fastq)
    one = gs.same_as_host(ctx, plain, fastq, want)
    a = len(text) // 2
    for small, window in ((1500, 1), (1, 1), (4097, 1), (1500, 20_000)):
        cuts = [a, a + small]
        blob = b"".join(members_of(text, cuts))
        gz = plain + ".gz"
        open(gz, "wb").write(blob)
        assert gzip.decompress(blob) == text
        check(ctx, gz, fastq, want, one, plain, listed(text, cuts), window, 1024)
        assert ctx.sequence_slice_info()["windows"] >= 4


def stored(text):
    return gs.member(text, 0)


def test_members_swapped_or_changed_between_index_and_slice_are_refused(ctx, tmp_path):
    """three stored members, the first two of the same size (so of the same compressed size): the file with those two exchanged has
    the size, the chain offsets and every ISIZE of the indexed one; so has the file with one inner CRC32 changed.  The slice refuses
    both, the context's reads stay the index's, and the unchanged file is sliced afterwards"""
    rec = [b">r%03d\n%s\n" % (k, b"ACGTTGCA" * (20 + k % 5)) for k in range(400)]
    a, b, c = b"".join(rec[:150]), b"".join(rec[150:300]), b"".join(rec[300:])
    assert len(a) == len(b) and a != b
    text = a + b + c
    plain = str(tmp_path / "abc.fasta")
    open(plain, "wb").write(text)
    want = host.host_read(plain, False)
    good = stored(a) + stored(b) + stored(c)
    swapped = stored(b) + stored(a) + stored(c)
    assert len(good) == len(swapped) and gzip.decompress(swapped) == b + a + c
    crc = bytearray(good)
    crc[len(stored(a)) - 8] ^= 1
    path = str(tmp_path / "abc.fasta.gz")
    everyone = np.arange(len(want["names"]))
    for window, chunk in ((0, 0), (3000, 1024)):
        open(path, "wb").write(good)
        ix = gs.same_as_host(ctx, path, False, want, window, chunk)
        assert ctx.gzip_members() == listed(text, [len(a), len(a) + len(b)])
        lens = want["length"]
        for name, data in (("swapped", swapped), ("crc", bytes(crc))):
            open(path, "wb").write(data)
            assert ctx.slice_sequences(path, everyone, ix["length"])[0] == 8, name
            # the reads are still the index's
            assert gs._mhap_check(ctx, tmp_path, int(lens[0]), int(lens[1])) == -1, name
            assert gs._mhap_check(ctx, tmp_path, int(lens[0]), int(lens[1]) + 1) == 1, name
        open(path, "wb").write(good)
        hashes, _ = gs.sliced(ctx, path, ix, everyone)
        assert hashes.tolist() == want["hash"].tolist()
    # indexing the swapped file is fine - it is a good file of its own - and indexing the one with the wrong CRC32 is refused
    open(path, "wb").write(swapped)
    gs.same_as_host(ctx, path, False, host.host_read(path, False))
    open(path, "wb").write(bytes(crc))
    assert gs.index(ctx, path, False)[0] == 8
    # with the option off a file of several members is refused as it ever was
    open(path, "wb").write(good)
    ctx.set_option("gzip_members", 0)
    try:
        assert gs.index(ctx, path, False)[0] == 8
    finally:
        ctx.set_option("gzip_members", 1)
    gs.same_as_host(ctx, path, False, want)


def _cli(exe, args, sequences, gz):
    env = dict(os.environ, RALA_DEVICE_SEQUENCES=sequences, RALA_DEVICE_GZIP=gz, RALA_HIP_TRACE="1")
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    return r.returncode, r.stdout, r.stderr.decode()


def test_cli_reads_and_overlaps_of_several_members(tmp_path):
    """rala reads.fastq.gz ovl.paf.gz, both `cat` of several .gz files: RALA_DEVICE_GZIP=2 takes both on the device and names the
    member counts; =1 hands both to the host reader; the contigs are those of both switches off"""
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    lines = open(fa, "rb").read().split(b"\n")
    pairs = [(lines[2 * i][1:], lines[2 * i + 1]) for i in range(ds.n_reads)]
    fq_text = host.fastq_text(pairs)
    fq = str(tmp_path / "reads.fastq.gz")
    cuts = cut_points(fq_text, True, 7, "record", seed=2)
    open(fq, "wb").write(b"".join(gzip.compress(t, 6) for t in (fq_text[a:b] for a, b in zip([0] + cuts, cuts + [len(fq_text)]))))
    paf_text = open(paf, "rb").read()
    ovl = str(tmp_path / "ovl.paf.gz")
    n = len(paf_text)
    open(ovl, "wb").write(b"".join(gzip.compress(paf_text[n * k // 5:n * (k + 1) // 5], 6) for k in range(5)))
    rc, out_off, err_off = _cli(exe, [fq, ovl], "0", "0")
    assert rc == 0 and len(out_off) > 1000, err_off[-2000:]
    rc, out_on, err_on = _cli(exe, [fq, ovl], "1", "2")
    assert rc == 0, err_on[-2000:]
    assert out_on == out_off
    assert "device inflate: 7 gzip members" in err_on and "device inflate: 5 gzip members" in err_on, err_on[-3000:]
    assert "device sequence index" in err_on and "device sequence slice" in err_on
    assert "(flags 0)" in err_on.split("device sequence slice")[1].split("\n")[0]
    rc, out_one, err_one = _cli(exe, [fq, ovl], "1", "1")
    assert rc == 0, err_one[-2000:]
    assert out_one == out_off and "gzip members" not in err_one and "device sequence slice" not in err_one
