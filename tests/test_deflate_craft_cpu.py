"""CPU: the handmade deflate streams of tests/deflate_craft.py are what they are meant to be.  For every case zlib's inflate
gives the text (valid) or refuses / does not finish (invalid); wrapped as a single-member .paf.gz and as a BGZF file, the host
reader (io_paf_parse, streamed) gives the plain file's columns or is not ok; and the coverage reports show that a case
reaches the branch it is there for - long codes really are the common ones, every symbol and every repeat count occurs.
tests/test_gpu_inflate_crafted.py holds the device inflaters to the same verdicts."""
import os

import numpy as np
import pytest

from rala_amd.synth import Dataset

import deflate_craft as dc
import test_ingest_cpu as host


class World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World()
    w.dir = tmp_path_factory.mktemp("craft")
    w.ds = Dataset(500, 20_000, 12)
    w.names = ["r%d" % i for i in range(w.ds.n_reads)]
    w.text, w.far_at = dc.paf_text(w.ds, str(w.dir / "all.paf"), 3000)
    w.plain = str(w.dir / "plain.paf")
    with open(w.plain, "wb") as f:
        f.write(w.text)
    w.want = host_columns(w, w.plain, 0)
    assert w.want is not None and len(w.want["a_id"]) == 3000
    m = w.marker = World()                      # marker_copies' own text
    m.dir, m.ds, m.names = w.dir, w.ds, w.names
    with open(str(w.dir / "all.paf"), "rb") as f:
        m.text = dc.marker_text(f.read(), 600)
    with open(str(w.dir / "marker.paf"), "wb") as f:
        f.write(m.text)
    m.want = host_columns(m, str(w.dir / "marker.paf"), 0)
    assert m.want is not None and len(m.want["a_id"]) == 600
    return w


def host_columns(w, path, mode=2):
    """the host reader on the file (mode 2: streamed through zlib) -> columns, or None where it is not ok"""
    L = host._lib()
    rl = np.ascontiguousarray(w.ds.read_len, dtype=np.uint32)
    h = L.io_paf_parse(path.encode(), "\n".join(w.names).encode(), rl.ctypes.data, len(w.names), 1, 2, mode)
    try:
        if not L.io_paf_ok(h):
            return None
        n = int(L.io_paf_size(h))
        cols = {f: np.zeros(n, dtype=np.uint32) for f in host.FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.io_paf_copy(h, *[cols[f].ctypes.data for f in host.FIELDS], cols["strand"].ctypes.data)
        assert L.io_paf_length_error(h) == -1
        return cols
    finally:
        L.io_paf_free(h)


def same(got, want):
    assert got is not None
    for f in want:
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), f


def overlaps_forced(w):
    """the OV:Z: runs give both forced matches at each of the six distances"""
    forced = dc.overlap_forces(w.text)
    for d in dc.OVERLAP_DISTS:
        assert (258, d) in forced.values() and (3, d) in forced.values(), d
    return forced


@pytest.mark.parametrize("name", list(dc.VALID) + list(dc.GZIP_ONLY))
def test_valid_case_is_what_zlib_and_the_host_reader_take(world, name):
    w = world
    encode = dict(dc.VALID, **dc.GZIP_ONLY)[name]
    if name == "marker_copies":
        w = w.marker
    body, rep = encode(w.text)
    assert dc.verdict(body) == w.text
    dc.covers(name, rep)
    if name == "overlapping_copies":
        forced = overlaps_forced(w)
        toks = dc.tokens_of(w.text, forced=forced)
        assert sum(t == f for t in toks for f in set(forced.values())) >= len(forced)
    gz = str(w.dir / (name + ".paf.gz"))
    with open(gz, "wb") as f:
        f.write(dc.gz_member(body, w.text))
    same(host_columns(w, gz), w.want)
    if name in dc.VALID:
        blob, rep = dc.bgzf_file(w.text, encode, cuts=[w.far_at])
        dc.covers(name, rep)
        with open(gz, "wb") as f:
            f.write(blob)
        same(host_columns(w, gz), w.want)


def test_bgzf_members_of_1_3_and_65536_bytes(world):
    w = world
    sizes = [1, 3, 65536]
    blob, rep = dc.bgzf_file(w.text, dc.long_lit_codes, size=lambda k: sizes[k % 3])
    assert rep["member_text"][:3] == sizes and rep["member_text"].count(65536) >= 1
    gz = str(w.dir / "sizes.paf.gz")
    with open(gz, "wb") as f:
        f.write(blob)
    same(host_columns(w, gz), w.want)


@pytest.mark.parametrize("place", dc.PLACES)
@pytest.mark.parametrize("name", dc.INVALID_NAMES)
def test_invalid_case_is_refused_by_zlib_and_the_host_reader(world, name, place):
    w = world
    body, _, got = dc.invalid(name, w.text, place)
    assert dc.verdict(body) is None
    gz = str(w.dir / ("%s_%s.paf.gz" % (name, place)))
    with open(gz, "wb") as f:
        f.write(dc.gz_member(body, got))
    assert host_columns(w, gz) is None
    with open(gz, "wb") as f:
        f.write(dc.bgzf_with_bad_member(w.text, name, place))
    assert host_columns(w, gz) is None


def test_code_length_shapes_are_complete():
    rng = np.random.default_rng(1)
    for n, used in ((286, 20), (286, 200), (30, 9), (30, 30), (19, 12)):
        freq = {int(s): int(rng.integers(1, 1000)) for s in rng.choice(n, used, replace=False)}
        limit = 7 if n == 19 else 15
        for lens in (dc.optimal(freq, n, limit), dc.deep(freq, n, 3, limit=limit), dc.comb(freq, n) if used <= 16 and limit == 15 else None):
            if lens is not None:
                assert dc.kraft(lens) == 1 << 15 and max(lens) <= limit and all(lens[s] for s in freq)
    assert sorted(l for l in dc.comb({s: 1 for s in range(16)}, 286) if l) == list(range(1, 16)) + [15]
    heavy = dc.deep({0: 1000, 1: 10, 2: 1}, 286, 1)
    assert heavy[0] == max(heavy) >= 11 and heavy[0] >= heavy[1] >= heavy[2] > 0
