"""GPU: the device inflaters (rala_amd/csrc/inflate_kernels.hip: bgzf_inflate_kernel; gzip find / count / write / windows /
resolve) on the handmade deflate streams of tests/deflate_craft.py - what zlib's inflate accepts but its compressor never
writes (long codes, one or no distance code, padded and minimal headers, every repeat count, every length and distance
symbol, copies that overlap themselves, stored and empty blocks, blocks that open with a match into text the wave has not
seen), and streams with one thing in them that zlib refuses.  The verdicts are zlib's and the host reader's
(tests/test_deflate_craft_cpu.py proves them for the same cases): a valid case gives the plain file's columns with no
flag - a fallback (flag 8) is a failure -, an invalid one gives flag 8 and no rows, and a context that refused files
parses good ones afterwards.  Every stream sent to the device is first given to zlib here, and every valid one's coverage
report is checked (dc.covers).  The gzip tests print the inflater's counts."""
import ctypes

import numpy as np
import pytest

from rala_amd import hip

from rala_amd.synth import Dataset

import deflate_craft as dc
import test_gpu_bgzf as gb
import test_gpu_gzip as gg
import test_gpu_ingest as gi

pytestmark = pytest.mark.gpu
CHUNKS = (1024, 4096, None)                 # gzip_chunk_bytes; None: the default
SEVERAL_WAVES = ("tiny_blocks", "long_lit_codes", "stored_mix", "stored_mix_65535", "marker_copies")


class World:
    def __init__(self, tmp, n_lines, seed, marker=False):
        self.dir = tmp
        self.ds = Dataset(500, 20_000, seed)
        self.names = ["r%d" % i for i in range(self.ds.n_reads)]
        self.text, self.far_at = dc.paf_text(self.ds, str(tmp / "all.paf"), n_lines)
        if marker:                              # marker_copies' text: every line ends in the three copies
            with open(str(tmp / "all.paf"), "rb") as f:
                self.text, self.far_at = dc.marker_text(f.read(), n_lines), 0
        self.plain = str(tmp / "plain.paf")
        with open(self.plain, "wb") as f:
            f.write(self.text)
        self.want, irregular, bad = gi.device_parse(self.plain, self.names, self.ds.read_len)
        assert irregular == 0 and bad == -1 and len(self.want["a_id"]) == n_lines

    def write(self, name, blob):
        path = str(self.dir / (name + ".paf.gz"))
        with open(path, "wb") as f:
            f.write(blob)
        return path


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("valid"), 8000, 12)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return World(tmp_path_factory.mktemp("small"), 3000, 13)


@pytest.fixture(scope="module")
def marker(tmp_path_factory):
    return World(tmp_path_factory.mktemp("marker"), 600, 12, marker=True)


def options(chunk):
    return {} if chunk is None else dict(gzip_chunk_bytes=chunk)


@pytest.mark.parametrize("name", list(dc.VALID))
def test_bgzf_valid_case_equals_the_plain_file(world, small, name):
    w = small if name == "tiny_blocks" else world
    blob, rep = dc.bgzf_file(w.text, dc.VALID[name], cuts=[w.far_at])
    dc.covers(name, rep)
    got, irregular, bad = gi.device_parse(w.write("bgzf_" + name, blob), w.names, w.ds.read_len)
    assert irregular == 0 and bad == -1, (name, irregular, bad)
    gb.same(got, w.want)


def test_bgzf_members_of_1_3_and_65536_bytes_under_long_codes(small):
    w = small
    sizes = [1, 3, 65536]
    blob, rep = dc.bgzf_file(w.text, dc.long_lit_codes, size=lambda k: sizes[k % 3])
    assert rep["member_text"][:3] == sizes
    got, irregular, bad = gi.device_parse(w.write("bgzf_sizes", blob), w.names, w.ds.read_len)
    assert irregular == 0 and bad == -1
    gb.same(got, w.want)


@pytest.mark.parametrize("name", list(dc.VALID) + list(dc.GZIP_ONLY))
def test_gzip_valid_case_equals_the_plain_file(world, small, marker, name):
    w = small if name == "tiny_blocks" else marker if name == "marker_copies" else world
    body, rep = dict(dc.VALID, **dc.GZIP_ONLY)[name](w.text)
    assert dc.verdict(body) == w.text
    dc.covers(name, rep)
    path = w.write("gzip_" + name, dc.gz_member(body, w.text))
    for chunk in CHUNKS:
        print(name, "chunk", chunk, end=" ")
        gz = gg.good(gg.device(path, w.names, w.ds.read_len, **options(chunk)), w.want, len(w.text))
        if chunk == 4096 and name in SEVERAL_WAVES:
            assert gz["confirmed"] >= 2, gz
        if name == "marker_copies" and chunk is not None:
            # dc.covers: at least 3 chunks' first blocks open with each of the three kinds of copy, and its blocks begin
            # nowhere else but every 4000 tokens - so with nearly every chunk confirmed, several starts of each kind are
            first = dc.chunk_first_blocks(rep["starts"], chunk)
            assert gz["refuted"] == 0 and gz["confirmed"] >= sum(first.values()) - 2, (gz, first)


def refused_by_bgzf(w, name, place):
    path = w.write("bad_bgzf_%s_%s" % (name, place), dc.bgzf_with_bad_member(w.text, name, place))
    info = gb.raw_device(path, w.names, w.ds.read_len)
    assert info[0] == 0 and info[1] & 8 and info[3] == 0, (name, place, info)


def refused_by_gzip(w, name, place):
    body, _, got = dc.invalid(name, w.text, place)
    assert dc.verdict(body) is None
    path = w.write("bad_gzip_%s_%s" % (name, place), dc.gz_member(body, got))
    for chunk in (4096, 1 << 22):
        res = gg.device(path, w.names, w.ds.read_len, gzip_chunk_bytes=chunk)
        print(name, place, "chunk", chunk, res[3])
        assert res[0] is None and res[1] & 8 and res[2] == -1 and res[4] == 0, (name, place, chunk, res[1:])


@pytest.mark.parametrize("place", dc.PLACES)
@pytest.mark.parametrize("name", dc.INVALID_NAMES)
def test_bgzf_invalid_case_is_flag_8_and_no_rows(small, name, place):
    refused_by_bgzf(small, name, place)


@pytest.mark.parametrize("place", dc.PLACES)
@pytest.mark.parametrize("name", dc.INVALID_NAMES)
def test_gzip_invalid_case_is_flag_8_and_no_rows(small, name, place):
    """(distance_before_text, last: a block reached by a wave other than the first copies from in front of the whole text -
    only the windows / resolve passes can see it)"""
    refused_by_gzip(small, name, place)


def through(ctx, path):
    """path (MHAP) through rala_hip_set_overlaps_from_mhap of the context -> (irregular, columns or None)"""
    bad, irregular = ctypes.c_int64(0), ctypes.c_int(0)
    f = ctx.L.rala_hip_set_overlaps_from_mhap
    f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    assert f(ctx.h, path.encode(), 1, 4, ctypes.byref(bad), ctypes.byref(irregular)) == 0
    assert bad.value == -1
    if irregular.value:
        return irregular.value, None
    g = ctx.L.rala_hip_get_overlap_columns
    g.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    n = ctypes.c_uint64(0)
    assert g(ctx.h, ctypes.byref(n), None, None) == 0
    cols = {f: np.zeros(n.value, dtype=np.uint32) for f in gg.FIELDS}
    cols["strand"] = np.zeros(n.value, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * 7)(*[cols[f].ctypes.data for f in gg.FIELDS])
    assert g(ctx.h, ctypes.byref(n), ptrs, cols["strand"].ctypes.data) == 0
    return 0, cols


def test_one_context_parses_good_files_after_rejected_ones(small):
    """one context (MHAP, which needs no name table): rejected streams of both kinds set flag 8, then zlib's own files give
    the plain file's columns from that same context - a refusal leaves it usable"""
    w = small
    mhap = str(w.dir / "ovl.mhap")
    gg.host._to_mhap(str(w.dir / "all.paf"), mhap)
    with open(mhap, "rb") as f:
        text = b"".join(f.read().splitlines(keepends=True)[:4000])
    with open(mhap, "wb") as f:
        f.write(text)
    want, irregular, bad = gi.device_parse_mhap(mhap, w.ds.read_len)
    assert irregular == 0 and bad == -1 and len(want["a_id"]) == 4000
    ctx = hip.Context(0)
    try:
        ctx.set_option("gzip_on_device", 1)
        ctx.set_option("gzip_chunk_bytes", 4096)
        ctx.set_reads(w.ds.read_len)
        for name in ("oversubscribed_ll", "distance_before_text", "stored_past_end"):
            body, _, got = dc.invalid(name, text, "last")
            assert dc.verdict(body) is None
            path = str(w.dir / ("bad_%s.mhap.gz" % name))
            for blob in (dc.gz_member(body, got), dc.bgzf_with_bad_member(text, name, "last")):
                with open(path, "wb") as f:
                    f.write(blob)
                irregular, cols = through(ctx, path)
                assert irregular & 8 and cols is None, (name, irregular)
            gg.write_gz(mhap, mhap + ".gz", level=6)
            irregular, cols = through(ctx, mhap + ".gz")
            assert irregular == 0
            gb.same(cols, want)
            gb.write_bgzf(mhap, mhap + ".gz", gb.random_sizes(3), level=6)
            irregular, cols = through(ctx, mhap + ".gz")
            assert irregular == 0
            gb.same(cols, want)
    finally:
        ctx.close()
