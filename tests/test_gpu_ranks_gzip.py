"""GPU: a single-member gzip overlap file that is not BGZF - what gzip, pigz and `minimap2 | gzip` write - taken by the ranks of
a sharded run TOGETHER (rala_hip_mg_set_overlaps_from_paf / _mhap with the options gzip_on_device and gzip_in_pieces on every
rank's slice context), ranks as threads on the one device.  The oracle is always the host reader's columns for the same file
(test_ingest_cpu.parse); for what is refused, zlib's verdict.  Slices back to back are the file's records, cuts are run
boundaries, a file the ranks cannot prove is irregular 8 on every rank with nothing set, and the group takes a good file
afterwards.  Every rank of a call gets the same options: no test here lets ranks disagree, makes a collective wait or provokes
a fault."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from rala_amd import build
from rala_amd.synth import Dataset

import deflate_craft as dc
import gzip_pieces_model as model
import test_gpu_bgzf as gb
import test_gpu_ingest as gi
import test_gpu_ranks_compressed as rc
import test_ingest_cpu as host

pytestmark = pytest.mark.gpu
# 1024 is the smallest chunk the driver accepts: every one of 8 ranks gets many chunks of a file of a few hundred KB
TOGETHER = {"gzip_on_device": 1, "gzip_in_pieces": 1, "gzip_chunk_bytes": 1024}
INFO = ("own_chunks", "own_jobs", "halo_jobs", "own_text_bytes", "window_markers", "longest_chase", "compose_us", "exchange_us")
NAMES40, LENS40 = rc.NAMES40, rc.LENS40


def together(path, names, read_len, world, mhap=False, options=TOGETHER, before=None, threads=2):
    """test_gpu_ranks_compressed.ranks, and every rank's rala_hip_get_gzip_pieces_info behind the call -> (columns of all ranks
    back to back or None, irregular, first length error, [(first record, records)], [info of rank k], (irregular, length
    error) of the file ingested before)"""
    import ctypes

    L = rc._lib()
    L.hp_paf_device_pieces_info.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    rl = np.ascontiguousarray(read_len, dtype=np.uint32)
    slices, share = np.zeros(2 * world, dtype=np.uint64), np.zeros(3 * world, dtype=np.uint64)
    keys = (ctypes.c_char_p * max(1, len(options)))(*[k.encode() for k in options])
    values = np.array(list(options.values()) or [0], dtype=np.int64)
    h = L.hp_text_device_ranks(path.encode(), before.encode() if before else None, "\n".join(names).encode(), rl.ctypes.data, len(rl), 1, threads,
                               world, int(mhap), 0, keys, values.ctypes.data, len(options), slices.ctypes.data, share.ctypes.data)
    try:
        info, was = np.zeros(6, dtype=np.int64), np.zeros(2, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        L.hp_paf_device_before(h, was.ctypes.data)
        assert info[0] == 0, info
        pieces = []
        for k in range(world):
            p = np.zeros(8, dtype=np.int64)
            assert L.hp_paf_device_pieces_info(h, k, p.ctypes.data) == 1
            pieces.append(dict(zip(INFO, (int(x) for x in p))))
        if info[1] or info[2] >= 0:
            return None, int(info[1]), int(info[2]), None, pieces, (int(was[0]), int(was[1]))
        n = int(info[3])
        cols = {f: np.zeros(n, dtype=np.uint32) for f in host.FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in host.FIELDS], cols["strand"].ctypes.data)
        return cols, 0, -1, [(int(slices[2 * k]), int(slices[2 * k + 1])) for k in range(world)], pieces, (int(was[0]), int(was[1]))
    finally:
        L.hp_paf_device_free(h)


def taken(path, names, lens, world, want, **kw):
    """the ranks take the file: irregular 0, the host reader's columns, cuts on run boundaries -> every rank's piece"""
    got, irregular, bad, slices, pieces, _ = together(path, names, lens, world, **kw)
    print(os.path.basename(path), "world", world, [(p["own_chunks"], p["own_jobs"], p["halo_jobs"], p["own_text_bytes"], p["window_markers"],
                                                   p["longest_chase"]) for p in pieces])
    assert irregular == 0 and bad == -1, (path, world, irregular, bad)
    gi._check_slices(got, slices, want)
    return pieces


def refused(path, good, names, lens, world, want, **kw):
    """irregular 8 on every rank with nothing set (hp_text_device_ranks checks both), then the good file on the same group"""
    got, irregular, bad, slices, _, was = together(good, names, lens, world, before=path, **kw)
    assert was == (8, -1), (path, was)
    assert irregular == 0 and bad == -1, path
    gi._check_slices(got, slices, want)


def gz_file(path, text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    """one gzip member around zlib's deflate of the text (flush_every: a block boundary after every so many bytes of it)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = b""
    if flush_every:
        for i in range(0, len(text), flush_every):
            body += c.compress(text[i:i + flush_every]) + c.flush(zlib.Z_BLOCK)
    else:
        body = c.compress(text)
    body += c.flush()
    open(path, "wb").write(dc.gz_member(body, text))
    return path


def host_columns(d, text, name="plain.paf"):
    path = str(d / name)
    open(path, "wb").write(text)
    want, e0 = host.parse(path, NAMES40, LENS40, 2, True)
    assert e0 == -1
    return want


@pytest.fixture(scope="module")
def c_small(tmp_path_factory):
    """Dataset(3000, 600_000, 4) as PAF and MHAP, by gzip -6 and by zlib at levels 1 and 9; the host reader's columns, computed once"""
    d = tmp_path_factory.mktemp("ranks_gzip")
    ds = Dataset(3000, 600_000, 4)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf, mhap = str(d / "ovl.paf"), str(d / "ovl.mhap")
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    files = {}
    for kind, plain in (("paf", paf), ("mhap", mhap)):
        text = open(plain, "rb").read()
        by_gzip = str(d / ("gzip6." + kind + ".gz"))
        with open(by_gzip, "wb") as f:
            subprocess.run(["gzip", "-6", "-c", plain], stdout=f, check=True)
        files[kind] = {"gzip -6": by_gzip, "zlib 1": gz_file(str(d / ("zlib1." + kind + ".gz")), text, 1),
                       "zlib 9": gz_file(str(d / ("zlib9." + kind + ".gz")), text, 9)}
    want_paf, e0 = host.parse(paf, names, ds.read_len, 2, True)
    want_mhap, e1 = host.parse(mhap, names, ds.read_len, 2, 3)
    assert e0 == -1 and e1 == -1
    return dict(ds=ds, names=names, lens=ds.read_len, paf=paf, mhap=mhap, files=files, want={"paf": want_paf, "mhap": want_mhap}, dir=d)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("writer", ["gzip -6", "zlib 1", "zlib 9"])
def test_gzip_paf_and_mhap_over_ranks(c_small, writer, world):
    """The main case.  It cannot pass with all the work on rank 0: every rank owns jobs, and every rank but the first resolved
    symbols of its own through the window composed from the ranks in front of it (PAF and MHAP text is full of matches that
    reach far back, so the first symbols of any piece are such markers)."""
    c = c_small
    for kind in ("paf", "mhap"):
        pieces = taken(c["files"][kind][writer], c["names"], c["lens"], world, c["want"][kind], mhap=kind == "mhap")
        assert all(p["own_jobs"] > 0 and p["own_chunks"] > 0 for p in pieces), pieces
        assert all(p["window_markers"] > 0 for p in pieces[1:]), pieces
        assert pieces[0]["window_markers"] == 0
        assert sum(p["own_text_bytes"] for p in pieces) == os.path.getsize(c[kind])


def test_option_off_is_irregular_8_as_before(c_small):
    """without gzip_in_pieces a gzip file that is not BGZF is refused on every rank, whatever else is set: the default is pinned"""
    c = c_small
    path = c["files"]["paf"]["gzip -6"]
    for options in ({"bgzf_in_pieces": 1}, {"bgzf_in_pieces": 1, "gzip_on_device": 1}, {"bgzf_in_pieces": 1, "gzip_on_device": 1, "gzip_in_pieces": 0},
                    {"bgzf_in_pieces": 1, "gzip_in_pieces": 1}):
        got, irregular, bad, _, pieces, _ = together(path, c["names"], c["lens"], 3, options=options)
        assert got is None and irregular == 8 and bad == -1, (options, irregular)
        assert all(p["own_chunks"] == 0 and p["own_jobs"] == 0 for p in pieces)


def test_small_pieces_compose_through_several_ranks(tmp_path):
    """a file of 8 - 16 chunks over 8 ranks: every piece's text is shorter than one window, so the window in front of a rank is
    composed from several ranks' out-windows, and some ranks own no job at all"""
    text = ("\n".join(rc.run_lines(14)[:1100]) + "\n").encode()
    want = host_columns(tmp_path, text)
    path = gz_file(str(tmp_path / "small.paf.gz"), text, 6, flush_every=7000)
    n_chunks = (os.path.getsize(path) - 18 + 1023) // 1024
    assert 8 <= n_chunks <= 16, n_chunks
    pieces = taken(path, NAMES40, LENS40, 8, want)
    assert all(p["own_text_bytes"] < model.WINDOW for p in pieces), pieces
    assert any(p["own_jobs"] == 0 for p in pieces) and sum(p["own_jobs"] > 0 for p in pieces) >= 4, pieces
    assert sum(p["own_text_bytes"] for p in pieces) == len(text)
    # a rank that took symbols from the window in front of it although the rank before it owns less than one window of text,
    # with text in front of that: what it took lay - for a rank behind one without any text, all of it - in an earlier
    # rank's text and came through more than one out-window (blocks of 7000 bytes of text in about 1 KB chunks leave a rank
    # or two in the middle without a block's start)
    front = np.concatenate(([0], np.cumsum([p["own_text_bytes"] for p in pieces])))
    through = [k for k in range(2, 8) if pieces[k]["window_markers"] > 0 and front[k - 1] > 0 and pieces[k - 1]["own_text_bytes"] < model.WINDOW]
    behind_nothing = [k for k in through if pieces[k - 1]["own_text_bytes"] == 0]
    assert through and behind_nothing, pieces


@pytest.mark.parametrize("world", [3, 8])
def test_long_distance_matches_across_every_rank_boundary(tmp_path, world):
    """lines that come back 20 000 - 32 768 bytes later (gzip_pieces_model.far_text; the idea of tests/test_gpu_sequences_gzip.py's
    generator, as valid PAF lines), block boundaries every few KB: matches of that distance cross every rank boundary, and
    the first boundary lies at a text offset below one window.  The text's size goes with the number of ranks so that it does:
    the first 20 000 bytes have nothing to repeat and compress worst, so rank 0's share of the compressed bytes - a third of
    about 14 KB for 100 000 bytes of text, an eighth of about 32 KB for 260 000 - ends 18 000 to 24 000 bytes into the text."""
    text = model.far_text({3: 100_000, 8: 260_000}[world], 7)
    want = host_columns(tmp_path, text)
    for level in (6, 9):
        path = gz_file(str(tmp_path / ("far%d.paf.gz" % level)), text, level, flush_every=6000)
        pieces = taken(path, NAMES40, LENS40, world, want)
        assert all(p["own_jobs"] > 0 for p in pieces), pieces
        assert all(p["window_markers"] > 0 for p in pieces[1:]), pieces
        assert 0 < pieces[0]["own_text_bytes"] < model.WINDOW, pieces[0]


def test_streams_where_rank_0_owns_everything(tmp_path):
    """no dynamic block, so no start to find: fixed codes, stored blocks; a file smaller than one chunk; an empty text"""
    text = ("\n".join(rc.run_lines(15)[:2500]) + "\n").encode()
    want = host_columns(tmp_path, text)
    for name, kw in (("fixed", dict(level=6, strategy=zlib.Z_FIXED)), ("stored", dict(level=0))):
        path = gz_file(str(tmp_path / (name + ".paf.gz")), text, **kw)
        assert os.path.getsize(path) > 8 * 1024
        for world in (2, 8):
            pieces = taken(path, NAMES40, LENS40, world, want)
            assert pieces[0]["own_jobs"] == 1 and pieces[0]["own_text_bytes"] == len(text), pieces
            assert all(p["own_jobs"] == 0 and p["own_text_bytes"] == 0 and p["own_chunks"] > 0 for p in pieces[1:]), pieces
    tiny = ("\n".join(rc.run_lines(16)[:8]) + "\n").encode()
    path = gz_file(str(tmp_path / "tiny.paf.gz"), tiny)
    assert os.path.getsize(path) < 1024
    pieces = taken(path, NAMES40, LENS40, 8, host_columns(tmp_path, tiny, "tiny.paf"))
    assert [p["own_jobs"] for p in pieces] == [1] + [0] * 7 and [p["own_chunks"] for p in pieces] == [1] + [0] * 7
    path = gz_file(str(tmp_path / "empty.paf.gz"), b"")
    pieces = taken(path, NAMES40, LENS40, 3, host_columns(tmp_path, b"", "empty.paf"))
    assert all(p["own_text_bytes"] == 0 for p in pieces)


@pytest.fixture(scope="module")
def good40(tmp_path_factory):
    d = tmp_path_factory.mktemp("good40")
    text = ("\n".join(rc.run_lines(17)[:4000]) + "\n").encode()
    return dict(dir=d, text=text, want=host_columns(d, text), path=gz_file(str(d / "good.paf.gz"), text, 6, flush_every=9000))


def zlib_takes(blob):
    """zlib's verdict on a whole file: one gzip member and nothing else, or not"""
    try:
        d = zlib.decompressobj(31)
        d.decompress(blob)
        return d.eof and not d.unused_data
    except zlib.error:
        return False


def test_refusals_are_irregular_8_on_every_rank_and_the_group_goes_on(good40, tmp_path):
    g = good40
    data = open(g["path"], "rb").read()
    n = len(data)
    assert zlib_takes(data) and n > 30 * 1024
    taken(g["path"], NAMES40, LENS40, 3, g["want"])
    cases = {}
    for k in range(3):                                          # a flipped byte inside each rank's range of the deflate bytes
        b = bytearray(data)
        b[10 + (n - 18) * (2 * k + 1) // 6] ^= 0x20
        cases["flip%d" % k] = bytes(b)
    cases["crc32"] = data[:-8] + struct.pack("<I", struct.unpack("<I", data[-8:-4])[0] ^ 1) + data[-4:]
    cases["isize"] = data[:-4] + struct.pack("<I", len(g["text"]) + 1)
    cases["cut"] = data[:n * 2 // 3]
    cases["behind"] = data + b"\n"
    cases["two_members"] = data + gzip.compress(b"r1\t1001\n", 6)
    for name, blob in cases.items():
        assert not zlib_takes(blob), name
        path = str(tmp_path / (name + ".paf.gz"))
        open(path, "wb").write(blob)
        refused(path, g["path"], NAMES40, LENS40, 3, g["want"])
    # a BGZF file with the two gzip options alone (no bgzf_in_pieces): refused, and not taken as the text it is not
    path = str(tmp_path / "bgzf.paf.gz")
    rc.write_members(g["text"], path, [20_000])
    refused(path, g["path"], NAMES40, LENS40, 3, g["want"])
    got, irregular, bad, _, _, _ = together(path, NAMES40, LENS40, 3)
    assert got is None and irregular == 8 and bad == -1


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = tmp_path_factory.mktemp("crafted")
    ds = Dataset(500, 20_000, 13)
    names = ["r%d" % i for i in range(ds.n_reads)]
    text, _ = dc.paf_text(ds, str(d / "all.paf"), 900)
    plain = str(d / "plain.paf")
    open(plain, "wb").write(text)
    want, e0 = host.parse(plain, names, ds.read_len, 2, True)
    assert e0 == -1
    good = gz_file(str(d / "good.paf.gz"), text, 6, flush_every=5000)
    return dict(dir=d, ds=ds, names=names, text=text, want=want, good=good)


@pytest.mark.parametrize("name", dc.INVALID_NAMES)
def test_crafted_invalid_streams_as_the_whole_file(crafted, name):
    """every "invalid" stream of tests/deflate_craft.py, the change in its first and in its last block: what zlib refuses is
    irregular 8 on every rank and the group goes on; what zlib takes (the verdict is zlib's, not the case's intention) must
    give the host reader's columns for zlib's text"""
    c = crafted
    for place in dc.PLACES:
        body, _, got = dc.invalid(name, c["text"], place)
        path = str(c["dir"] / ("%s_%s.paf.gz" % (name, place)))
        open(path, "wb").write(dc.gz_member(body, got))
        if dc.verdict(body) is None:
            refused(path, c["good"], c["names"], c["ds"].read_len, 3, c["want"])
        else:
            plain = str(c["dir"] / ("%s_%s.paf" % (name, place)))
            open(plain, "wb").write(dc.verdict(body))
            want, e0 = host.parse(plain, c["names"], c["ds"].read_len, 2, True)
            taken(path, c["names"], c["ds"].read_len, 3, want)


def test_cli_over_two_ranks_from_a_gzip_file(tmp_path):
    """rala --gpus 2 from a .paf.gz by gzip -6: with RALA_DEVICE_COMPRESSED=1 RALA_DEVICE_GZIP=1 both ranks inflate a piece on the
    device; stdout and the stage lines (the simplify counts among them) are those of the run without the switches, where
    nothing is inflated there; RALA_DEVICE_INGEST=0 overrides both, RALA_DEVICE_GZIP=2 over ranks stays with the host"""
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    with open(paf + ".gz", "wb") as f:
        subprocess.run(["gzip", "-6", "-c", paf], stdout=f, check=True)
    two = dict(os.environ, RALA_COMM="local", RALA_GPU_DEVICES="0,0", RALA_HIP_TRACE="1")
    for k in ("RALA_DEVICE_COMPRESSED", "RALA_DEVICE_GZIP", "RALA_DEVICE_INGEST"):
        two.pop(k, None)

    def run(env):
        r = subprocess.run(["timeout", "-k", "10", "300", exe, "--gpus", "2", fa, paf + ".gz"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        err = r.stderr.decode()
        assert r.returncode == 0, err[-3000:]
        stages = [re.sub(r" \d+\.\d+ s$", "", x) for x in err.splitlines() if x.startswith("[rala::")]
        return r.stdout, stages, err

    off = run(two)
    on = run(dict(two, RALA_DEVICE_COMPRESSED="1", RALA_DEVICE_GZIP="1"))
    assert len(off[0]) > 1000 and any("simplif" in s.lower() for s in off[1]), off[1]
    assert on[:2] == off[:2]
    assert len(re.findall(r"device inflate: part \d of 2 of one gzip member", on[2])) == 2, on[2][-3000:]
    assert "device inflate" not in off[2]
    for env in (dict(RALA_DEVICE_COMPRESSED="1", RALA_DEVICE_GZIP="1", RALA_DEVICE_INGEST="0"), dict(RALA_DEVICE_COMPRESSED="1", RALA_DEVICE_GZIP="2"),
                dict(RALA_DEVICE_GZIP="1"), dict(RALA_DEVICE_COMPRESSED="1")):
        got = run(dict(two, **env))
        assert got[:2] == off[:2] and "device inflate" not in got[2], env
