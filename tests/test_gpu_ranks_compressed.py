"""GPU: the device ingest of a sharded run for BGZF and MHAP files (rala_hip_mg_set_overlaps_from_paf / _mhap with the option
"bgzf_in_pieces": rank k takes the members whose header begins in its byte range of the file) and of a compressed or MHAP
-s file (rala_hip_tokenise_sensitive), ranks as threads on the one device.  The oracle is always the host reader's columns
for the same file (test_ingest_cpu.parse): slices back to back are the file's records, cuts are run boundaries, a file the
pieces cannot prove is irregular 8 on every rank with nothing set, and the group takes a good file afterwards."""
import ctypes
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

import test_bgzf_pieces_cpu as pieces_cpu
import test_gpu_bgzf as gb
import test_gpu_ingest as gi
import test_ingest_cpu as host

pytestmark = pytest.mark.gpu
FIELDS = host.FIELDS
PIECES = {"bgzf_in_pieces": 1}


def _lib():
    L = gi._lib()
    L.hp_text_device_ranks.restype = ctypes.c_void_p
    L.hp_text_device_ranks.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                       ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.hp_paf_device_before.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def ranks(path, names, read_len, world, mhap=False, options=PIECES, before=None, sensitive=False, threads=2, check_lengths=True):
    """-> (columns of all ranks back to back or None, irregular, first length error, [(first record, records)], [(begin, end,
    empty)] of the -s shares, (irregular, length error) of the file ingested before)"""
    L = _lib()
    rl = np.ascontiguousarray(read_len, dtype=np.uint32)
    slices, share = np.zeros(2 * world, dtype=np.uint64), np.zeros(3 * world, dtype=np.uint64)
    keys = (ctypes.c_char_p * max(1, len(options)))(*[k.encode() for k in options])
    values = np.array(list(options.values()) or [0], dtype=np.int64)
    h = L.hp_text_device_ranks(path.encode(), before.encode() if before else None, "\n".join(names).encode(), rl.ctypes.data, len(rl),
                               int(check_lengths), threads, world, int(mhap), int(sensitive), keys, values.ctypes.data, len(options),
                               slices.ctypes.data, share.ctypes.data)
    try:
        info, was = np.zeros(6, dtype=np.int64), np.zeros(2, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        L.hp_paf_device_before(h, was.ctypes.data)
        assert info[0] == 0, info
        shares = [tuple(int(x) for x in share[3 * k:3 * k + 3]) for k in range(world)]
        if info[1] or info[2] >= 0:
            return None, int(info[1]), int(info[2]), None, shares, (int(was[0]), int(was[1]))
        n = int(info[3])
        cols = {f: np.zeros(n, dtype=np.uint32) for f in FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in FIELDS], cols["strand"].ctypes.data)
        return cols, 0, -1, [(int(slices[2 * k]), int(slices[2 * k + 1])) for k in range(world)], shares, (int(was[0]), int(was[1]))
    finally:
        L.hp_paf_device_free(h)


def write_members(data, dst, sizes, eof=True, **kw):
    """data's bytes as BGZF members of sizes[i] bytes of text (a list, cycled, zeros are empty members; or a function of i)"""
    out, i, k = [], 0, 0
    while i < len(data):
        n = sizes(k) if callable(sizes) else sizes[k % len(sizes)]
        out.append(gb.member(data[i:i + n], **kw))
        i += n
        k += 1
    if eof:
        out.append(gb.member(b""))
    open(dst, "wb").write(b"".join(out))
    return out


def taken(path, names, lens, world, want, mhap=False, **kw):
    """the ranks take the file: irregular 0, the host reader's columns, cuts on run boundaries"""
    got, irregular, bad, slices, _, _ = ranks(path, names, lens, world, mhap=mhap, **kw)
    assert irregular == 0 and bad == -1, (path, world, irregular, bad)
    gi._check_slices(got, slices, want)
    return slices


@pytest.fixture(scope="module")
def c_small(tmp_path_factory):
    """Dataset(3000, 600_000, 4) as PAF and MHAP, plain and BGZF with ragged members; the host reader's columns, computed once"""
    d = tmp_path_factory.mktemp("ranks_compressed")
    ds = Dataset(3000, 600_000, 4)
    names = ["r%d" % i for i in range(ds.n_reads)]
    paf, mhap = str(d / "ovl.paf"), str(d / "ovl.mhap")
    ds.write_paf(paf)
    host._to_mhap(paf, mhap)
    gb.write_bgzf(paf, paf + ".gz", gb.random_sizes(21))
    gb.write_bgzf(mhap, mhap + ".gz", gb.random_sizes(22), eof=False)
    want_paf, e0 = host.parse(paf, names, ds.read_len, 2, True)
    want_mhap, e1 = host.parse(mhap, names, ds.read_len, 2, 3)
    assert e0 == -1 and e1 == -1
    return dict(ds=ds, names=names, lens=ds.read_len, paf=paf, mhap=mhap, want_paf=want_paf, want_mhap=want_mhap, dir=d)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_bgzf_paf_and_mhap_and_plain_mhap_over_ranks(c_small, world):
    c = c_small
    slices = taken(c["paf"] + ".gz", c["names"], c["lens"], world, c["want_paf"])
    assert all(n_k > 0 for _, n_k in slices)
    taken(c["mhap"] + ".gz", c["names"], c["lens"], world, c["want_mhap"], mhap=True)
    # a plain .mhap over the ranks, with the option and without it
    taken(c["mhap"], c["names"], c["lens"], world, c["want_mhap"], mhap=True)
    taken(c["mhap"], c["names"], c["lens"], world, c["want_mhap"], mhap=True, options={})
    # (a plain .paf through the new entry's path is what it was)
    taken(c["paf"], c["names"], c["lens"], world, c["want_paf"])


NAMES40, LENS40 = ["r%d" % i for i in range(40)], [1000 + i for i in range(40)]


def rec(a, b, k, aname=None, bname=None):
    return "%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t400\t%d\t255" % (aname or "r%d" % a, LENS40[a], k % 90, 500 + k % 300, bname or "r%d" % b,
                                                                  LENS40[b], k % 80, 480 + k % 200, 450 + k % 50)


def run_lines(seed=11):
    """tests/test_gpu_ingest.py::test_byte_ranges_with_unresolved_names_long_runs_and_empty_ranks' file: records that do not
    resolve, two runs longer than a rank's share"""
    rng = np.random.default_rng(seed)
    lines, k = [], 0
    for a in range(40):
        run = 3000 if a in (7, 8) else int(rng.integers(1, 60))
        for _ in range(run):
            b = int(rng.integers(0, 40))
            what = rng.random()
            if what < 0.04:
                lines.append(rec(a, b, k, aname="nobody%d" % k))
            elif what < 0.08:
                lines.append(rec(a, b, k, bname="nothing"))
            else:
                lines.append(rec(a, b, k))
            k += 1
    return lines


def host_columns(tmp_path, text, name="plain.paf"):
    path = str(tmp_path / name)
    open(path, "wb").write(text)
    want, e0 = host.parse(path, NAMES40, LENS40, 2, True)
    assert e0 == -1
    return want


def test_tiny_members_unresolved_names_long_runs_and_empty_ranks(tmp_path):
    """members of 1 to 300 bytes of text: many members per line, lines and runs across several pieces, ranks that keep nothing"""
    text = ("\n".join(run_lines()) + "\n").encode()
    want = host_columns(tmp_path, text)
    path = str(tmp_path / "tiny.paf.gz")
    write_members(text, path, gb.random_sizes(3, 300), level=0)
    for world in (2, 3, 5, 8):
        slices = taken(path, NAMES40, LENS40, world, want)
    assert any(n_k == 0 for _, n_k in slices)
    # no newline at the end, members of a few bytes, compressed
    write_members(text[:-1], path, gb.random_sizes(4, 40), eof=False, level=6)
    taken(path, NAMES40, LENS40, 3, want)


def test_full_members_few_members_and_ranks_without_a_header(tmp_path):
    lines = run_lines(12)
    text = ("\n".join(lines) + "\n").encode()
    assert len(text) > 3 * 65536
    want = host_columns(tmp_path, text)
    path = str(tmp_path / "full.paf.gz")
    # members of exactly 65536 bytes of text
    members = write_members(text, path, [65536], level=6)
    assert struct.unpack("<I", members[0][-4:])[0] == 65536
    for world in (2, 3, 8):
        taken(path, NAMES40, LENS40, world, want)
    # fewer members than ranks: three (and the end marker) over eight
    small = text[:150_000]
    small = small[:small.rfind(b"\n") + 1]
    want_small = host_columns(tmp_path, small, "small.paf")
    members = write_members(small, path, [50_000], level=6)
    assert len(members) == 4
    taken(path, NAMES40, LENS40, 8, want_small)
    # ranks 1 .. P - 2 hold no header start: one stored member of 65000 bytes, a small one and the end marker over four ranks
    two = text[:65_000 + 3000]
    two = two[:two.rfind(b"\n") + 1]
    want_two = host_columns(tmp_path, two, "two.paf")
    write_members(two, path, [65_000], level=0)
    data = open(path, "rb").read()
    F = len(data)
    empty = [pieces_cpu.device_piece(data, pieces_cpu.split(F, 4, k), pieces_cpu.split(F, 4, k + 1))[3] for k in range(4)]
    assert empty == [False, True, True, False]
    taken(path, NAMES40, LENS40, 4, want_two)


def _tune(build_file, path):
    """pad the last line's tag until piece 1 of 2 begins exactly at its range's start -> (the file's bytes, that member's number)"""
    members = build_file(0)
    F, at, j = sum(len(m) for m in members), 0, 0
    while at < F // 2:
        at += len(members[j])
        j += 1
    assert 0 < j < len(members) - 2
    for pad in range(0, 1000):
        data = b"".join(build_file(pad))
        if len(data) // 2 == at:
            open(path, "wb").write(data)
            assert pieces_cpu.device_piece(data, at, len(data))[1] == at
            return data, j
    raise AssertionError("no padding puts the range's start on the member")


def test_both_sides_of_the_ownership_rule_at_a_range_start(tmp_path):
    """a line whose first byte is a member's first byte at a range's start belongs to the piece in front (which holds the
    newline, its member's last byte); one behind a newline that is the member's first byte belongs to the piece itself"""
    lines = [rec(k % 40, (k * 7) % 40, k) for k in range(200)]
    path = str(tmp_path / "own.paf.gz")
    for newline_first in (False, True):
        def build_file(pad):
            body = lines[:-1] + [lines[-1] + "\tzz:Z:" + "x" * pad]
            if newline_first:                       # every member but the first starts with the newline of the line in front
                texts = [body[0].encode()] + [("\n" + l).encode() for l in body[1:]] + [b"\n"]
            else:
                texts = [(l + "\n").encode() for l in body]
            return [gb.member(t, level=0) for t in texts] + [gb.member(b"")]
        data, j = _tune(build_file, path)           # (member j holds line j)
        want = host_columns(tmp_path, gzip.decompress(data), "own%d.paf" % newline_first)
        assert len(want["a_id"]) == 200
        got, irregular, bad, slices, _, _ = ranks(path, NAMES40, LENS40, 2)
        assert irregular == 0 and bad == -1
        for f in want:
            assert (got[f] == want[f]).all(), f
        # -s shares make no cuts: the rows of a share are the lines its piece owns - line j is in the first member of piece 1
        got, irregular, bad, slices, shares, _ = ranks(path, NAMES40, LENS40, 2, sensitive=True)
        assert irregular == 0 and shares[1][0] == len(data) // 2
        for f in want:
            assert (got[f] == want[f]).all(), f
        assert slices[0][1] == (j if newline_first else j + 1) and slices[0][1] + slices[1][1] == 200


def test_empty_members_at_the_ends_of_pieces_and_a_long_tag_line(tmp_path):
    lines = run_lines(13)[:2000]
    text = ("\n".join(lines) + "\n").encode()
    want = host_columns(tmp_path, text)
    path = str(tmp_path / "empty.paf.gz")
    write_members(text, path, [0, 150, 0], level=0)
    data = open(path, "rb").read()
    F = len(data)
    for world in (2, 3, 8):
        first_empty = last_empty = False
        for k in range(world):
            p = pieces_cpu.device_piece(data, pieces_cpu.split(F, world, k), pieces_cpu.split(F, world, k + 1))
            assert p[0] and not p[3]
            first_empty = first_empty or p[4][0][2] == 0
            last_empty = last_empty or p[4][-1][2] == 0
        assert first_empty and last_empty
        taken(path, NAMES40, LENS40, world, want)
    # one line of 300 000 bytes of tag across the pieces (stored members: the file's bytes are the text's)
    tag = (rec(1, 2, 5) + "\n" + rec(1, 3, 6) + "\tzz:Z:" + "x" * 300_000 + "\n" + rec(2, 3, 7) + "\n").encode()
    want_tag = host_columns(tmp_path, tag, "tag.paf")
    write_members(tag, path, gb.random_sizes(6, 3000), level=0)
    taken(path, NAMES40, LENS40, 8, want_tag)


def test_the_same_verdict_on_every_rank(tmp_path):
    lines = run_lines()
    bad_lines = list(lines)
    bad_lines[len(lines) * 3 // 4] = "r1\t999\t0\t500\t+\tr2\t1002\t0\t500\t400\t500\t255"
    path = str(tmp_path / "verdict.paf.gz")
    write_members(("\n".join(bad_lines) + "\n").encode(), path, gb.random_sizes(7, 5000), level=1)
    got, irregular, bad, _, _, _ = ranks(path, NAMES40, LENS40, 3)
    assert got is None and irregular == 0 and bad == 1
    bad_lines[len(lines) // 5] = "short\tline"
    write_members(("\n".join(bad_lines) + "\n").encode(), path, gb.random_sizes(7, 5000), level=1)
    got, irregular, bad, _, _, _ = ranks(path, NAMES40, LENS40, 3)
    assert got is None and irregular != 0 and irregular < (1 << 20)          # (bit 20: the ranks disagreed)


def header_shaped_paf():
    """the CPU test's file as a PAF: a stored member whose text holds, in a tag, a complete member header - the first
    candidate of piece 1 of 2"""
    lines = [rec(k % 40, (k * 3) % 40, k) for k in range(700)]
    for k in range(64):
        fake = gb.member(b"text that looks like a member %d" % k)
        if b"\n" not in fake and b"\r" not in fake:
            break
    first = gb.member(("\n".join(lines[:200]) + "\n").encode(), level=6)
    stored_text = ("\n".join(lines[200:500])).encode() + b"\tzz:Z:" + fake + b"\n"
    stored = gb.member(stored_text, level=0)
    last = gb.member(("\n".join(lines[500:]) + "\n").encode(), level=6)
    data = first + stored + last + gb.member(b"")
    fake_at = data.find(fake)
    assert len(first) < len(data) // 2 <= fake_at
    return data


def test_refusals_are_irregular_8_on_every_rank_and_the_group_goes_on(c_small, tmp_path):
    c = c_small
    ds, names, lens = c["ds"], c["names"], c["lens"]
    good = str(tmp_path / "good.paf.gz")
    text = open(c["paf"], "rb").read()
    members = write_members(text, good, [40_000])
    data = open(good, "rb").read()
    k = len(members) // 2
    at = sum(len(m) for m in members[:k])
    cases = {}
    b = bytearray(data)
    b[at + 18 + len(members[k]) // 3] ^= 0x55                       # inside a member's deflate bytes: CRC32 / ISIZE say so
    cases["crc"] = bytes(b)
    b = bytearray(data)
    b[at + 16] ^= 0x10                                              # BSIZE
    cases["bsize"] = bytes(b)
    cases["cut"] = data[:at + 100]
    cases["plain_gzip"] = gzip.compress(text[:2_000_000], 6)
    for name, blob in cases.items():
        path = str(tmp_path / (name + ".paf.gz"))
        open(path, "wb").write(blob)
        got, irregular, bad, slices, _, was = ranks(good, names, lens, 3, before=path)
        assert was == (8, -1), (name, was)
        assert irregular == 0 and bad == -1, name
        gi._check_slices(got, slices, c["want_paf"])
        got, irregular, bad, _, _, _ = ranks(path, names, lens, 3)
        assert got is None and irregular == 8 and bad == -1, (name, irregular)
    # the header-shaped string: a BGZF file to one context and to the host reader, refused by two pieces, taken by three
    path = str(tmp_path / "shaped.paf.gz")
    open(path, "wb").write(header_shaped_paf())
    want, e0 = host.parse(path, NAMES40, LENS40, 2, 2)
    assert e0 == -1 and len(want["a_id"]) == 700
    whole, irregular, bad = gi.device_parse(path, NAMES40, LENS40)
    assert irregular == 0 and bad == -1 and (whole["a_id"] == want["a_id"]).all()
    got, irregular, bad, _, _, _ = ranks(path, NAMES40, LENS40, 2)
    assert got is None and irregular == 8
    got, irregular, bad, _, _, _ = ranks(path, NAMES40, LENS40, 2, sensitive=True, check_lengths=False)
    assert got is None and irregular == 8
    small = str(tmp_path / "small.paf.gz")
    small_text = ("\n".join(run_lines(14)[:500]) + "\n").encode()
    write_members(small_text, small, [3000])
    got, irregular, bad, slices, _, was = ranks(small, NAMES40, LENS40, 2, before=path)
    assert was == (8, -1) and irregular == 0
    gi._check_slices(got, slices, host_columns(tmp_path, small_text, "small.paf"))
    # the option left at 0: a BGZF file is the text it is not, today's answer - the one the entry gave before it knew of pieces
    old = gi.device_parse_ranks(good, names, lens, 3)
    got, irregular, bad, _, _, _ = ranks(good, names, lens, 3, options={})
    assert got is None and old[0] is None and irregular == old[1] != 0 and bad == old[2]


@pytest.mark.parametrize("mhap", [False, True])
def test_sensitive_shares_of_plain_bgzf_and_gzip_files(c_small, tmp_path, mhap):
    """rala_hip_tokenise_sensitive: parts 1 and 3 of a plain and a BGZF file, the whole of a gzip -6 file; nobody looks at the
    reads' lengths; all shares together are the host reader's columns"""
    c = c_small
    plain = c["mhap"] if mhap else c["paf"]
    want = c["want_mhap"] if mhap else c["want_paf"]
    wrong = np.array(c["lens"], copy=True)
    wrong[5] += 1
    gz = str(tmp_path / ("sens.mhap.gz" if mhap else "sens.paf.gz"))
    open(gz, "wb").write(gzip.compress(open(plain, "rb").read(), 6))
    for parts in (1, 3):
        for path in (plain, plain + ".gz"):
            got, irregular, bad, _, shares, _ = ranks(path, c["names"], wrong, parts, mhap=mhap, sensitive=True, options={})
            assert irregular == 0 and bad == -1, (path, parts)
            for f in want:
                assert (got[f] == want[f]).all(), (path, parts, f)
            assert pieces_cpu.chain([(True,) + s for s in shares], os.path.getsize(path))
    got, irregular, bad, _, _, _ = ranks(gz, c["names"], wrong, 1, mhap=mhap, sensitive=True, options={"gzip_on_device": 1})
    assert irregular == 0 and bad == -1
    for f in want:
        assert (got[f] == want[f]).all(), f
    # a gzip file that is not BGZF: in parts, or without the option, it is the host reader's
    assert ranks(gz, c["names"], wrong, 3, mhap=mhap, sensitive=True, options={"gzip_on_device": 1})[1] == 8
    assert ranks(gz, c["names"], wrong, 1, mhap=mhap, sensitive=True, options={})[1] == 8


def test_a_refused_sensitive_call_leaves_the_context_to_construct(c_small, tmp_path):
    c = c_small
    want = gb._mhap_graph(c["mhap"], c["lens"])
    gz = str(tmp_path / "sens.mhap.gz")
    open(gz, "wb").write(gzip.compress(open(c["mhap"], "rb").read()[:500_000], 6))
    broken = bytearray(open(c["mhap"] + ".gz", "rb").read())
    broken[len(broken) * 3 // 4] ^= 0x5A
    bad_bgzf = str(tmp_path / "broken.mhap.gz")
    open(bad_bgzf, "wb").write(bytes(broken))
    ctx = hip.Context(0)
    try:
        ctx.set_reads(c["lens"])
        bad, irregular, n = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_uint64(0)
        f = ctx.L.rala_hip_set_overlaps_from_mhap
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        assert f(ctx.h, c["mhap"].encode(), 1, 8, ctypes.byref(bad), ctypes.byref(irregular)) == 0
        assert bad.value == -1 and irregular.value == 0
        assert ctx.L.rala_hip_get_overlap_columns(ctx.h, ctypes.byref(n), None, None) == 0
        ctx.n_overlaps = n.value
        ctx.initialize()
        s = ctx.L.rala_hip_tokenise_sensitive
        s.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        out, piece = hip.OverlapsC(), (ctypes.c_uint64 * 3)()
        for path, part, parts in ((gz, 0, 1), (gz, 1, 3), (bad_bgzf, 0, 1), (bad_bgzf, 1, 2)):
            assert s(ctx.h, path.encode(), 1, part, parts, 4, ctypes.byref(out), ctypes.byref(n), piece, ctypes.byref(irregular)) == 0
            assert irregular.value == 8 and n.value == 0, (path, part, parts)
        assert s(ctx.h, gz.encode(), 2, 0, 1, 4, ctypes.byref(out), ctypes.byref(n), piece, ctypes.byref(irregular)) != 0     # no such format
        ctx.construct()
        n_tr = ctx.remove_transitive_edges()
        got = (n_tr, ctx.graph(), ctx.piles(), ctx.valid(), ctx.pile_row_digests())
    finally:
        ctx.close()
    assert got[0] == want[0] and got[0] > 0
    for x, y in zip(got[1:3], want[1:3]):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


def test_graph_and_cli_over_two_ranks_from_bgzf_files(tmp_path):
    """rala --gpus 2 with RALA_DEVICE_COMPRESSED=1 on a BGZF primary file and a BGZF -s file: the graph (debug CSV and JSON)
    and the contigs are those of the same run from plain text; with the switch off the same bytes and the same stage lines,
    and no rank inflates anything"""
    from oracle.oracle import Oracle

    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf, sens = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf"), str(tmp_path / "sens.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    o = Oracle(ds.read_len, ds.overlaps, n_threads=4)
    assert o.initialize() == 0
    o.pass2()
    o.preprocess_chimeras()
    p = o.piles()
    ds.sensitive(p["alive"], p["begin"], p["end"])
    ds.write_paf(sens, sensitive=True, target_len=(p["end"] - p["begin"]).astype(np.uint32))
    gb.write_bgzf(paf, paf + ".gz", gb.random_sizes(31))
    gb.write_bgzf(sens, sens + ".gz", gb.random_sizes(32))
    two = dict(os.environ, RALA_COMM="local", RALA_GPU_DEVICES="0,0", RALA_HIP_TRACE="1")
    two.pop("RALA_DEVICE_COMPRESSED", None)

    def run(primary, sensitive, env, tag):
        prefix = str(tmp_path / tag)
        r = subprocess.run([exe, "-u", "-d", prefix, "-s", sensitive, "--gpus", "2", fa, primary], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=600)
        err = r.stderr.decode()
        assert r.returncode == 0, err[-3000:]
        stages = [re.sub(r" \d+\.\d+ s$", "", x) for x in err.splitlines() if x.startswith("[rala::")]
        return r.stdout, open(prefix + ".csv").read(), open(prefix + ".json").read(), stages, err

    text = run(paf, sens, two, "text")
    on = run(paf + ".gz", sens + ".gz", dict(two, RALA_DEVICE_COMPRESSED="1"), "on")
    off = run(paf + ".gz", sens + ".gz", two, "off")
    assert len(text[0]) > 1000
    for got in (on, off):
        assert got[:4] == text[:4]
    # four pieces were inflated on the device with the switch on - two of the primary file, two of the -s file -, none without it
    assert len(re.findall(r"device inflate: part \d of 2", on[4])) == 4, on[4][-3000:]
    assert "device inflate" not in off[4]
    # RALA_DEVICE_INGEST=0 overrides the switch
    none = run(paf + ".gz", sens + ".gz", dict(two, RALA_DEVICE_COMPRESSED="1", RALA_DEVICE_INGEST="0"), "none")
    assert none[:4] == text[:4] and "device inflate" not in none[4]
