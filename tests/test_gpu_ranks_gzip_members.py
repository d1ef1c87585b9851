"""GPU: gzip overlap files of SEVERAL members that are not BGZF (cat part*.paf.gz, pigz -i) taken by the ranks of a sharded run
TOGETHER: rala_hip_mg_set_overlaps_from_paf / _mhap with the options gzip_on_device, gzip_in_pieces and gzip_members on every
rank's slice context, ranks as threads on the one device, chunks of 1024 compressed bytes.  The oracle is the host reader's
columns for the same bytes (test_ingest_cpu.parse); for what is refused, zlib's verdict member by member
(test_gpu_gzip_members.zlib_takes).  A good file gives irregular 0, slices that are the file's records back to back with cuts on
run boundaries, and the same member list on every rank; a file zlib refuses is irregular 8 on every rank with nothing set, and
the group takes a good file afterwards.  Every rank of a call gets the same options; nothing here makes a collective wait or
provokes a fault."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from rala_amd.synth import Dataset

import deflate_craft as dc
import test_gpu_gzip_members as gm
import test_gpu_ingest as gi
import test_gpu_ranks_compressed as rc
import test_gpu_ranks_gzip as rg
import test_ingest_cpu as host

pytestmark = pytest.mark.gpu
MEMBERS = dict(rg.TOGETHER, gzip_members=1)
CHUNK = 1024
MINFO = ("own_candidates", "members_begun", "member_ends", "registers_sent", "floor_stops", "compose_us")
member, listed, cut, line_starts = gm.member, gm.listed, gm.cut, gm.line_starts


def blocks(text, level=6, every=7000):
    """a member whose deflate stream has a block boundary after every `every` bytes of its text, as pigz writes them: a member of
    a few hundred KB by zlib alone is one or two blocks, which is one or two jobs however many ranks there are"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    body = b"".join(c.compress(text[i:i + every]) + c.flush(zlib.Z_BLOCK) for i in range(0, len(text), every)) + c.flush()
    return dc.gz_member(body, text)


def ranks(path, names, read_len, world, mhap=False, options=MEMBERS, before=None, threads=2):
    """hp_text_device_ranks, and what every rank's slice context says behind the call -> dict: cols (all ranks' back to back, or
    None), irregular, bad, slices, pieces / members_info (rala_hip_get_gzip_pieces_info / _member_pieces_info per rank), members
    (rala_hip_get_gzip_members per rank), was (irregular, length error of the file ingested before)"""
    L = rc._lib()
    L.hp_paf_device_pieces_info.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    L.hp_paf_device_member_pieces_info.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    L.hp_paf_device_rank_members.restype = ctypes.c_uint64
    L.hp_paf_device_before_rc.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    L.hp_paf_device_rank_members.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64] + [ctypes.c_void_p] * 3
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
        out = dict(cols=None, irregular=int(info[1]), bad=int(info[2]), slices=None, pieces=[], members_info=[], members=[],
                   was=(int(was[0]), int(was[1])), before_rc=[int(L.hp_paf_device_before_rc(h, k)) for k in range(world)])
        for k in range(world):
            p, m = np.zeros(8, dtype=np.int64), np.zeros(6, dtype=np.int64)
            assert L.hp_paf_device_pieces_info(h, k, p.ctypes.data) == 1 and L.hp_paf_device_member_pieces_info(h, k, m.ctypes.data) == 1
            out["pieces"].append(dict(zip(rg.INFO, (int(x) for x in p))))
            out["members_info"].append(dict(zip(MINFO, (int(x) for x in m))))
            n_m = L.hp_paf_device_rank_members(h, k, 0, None, None, None)
            off, size, crc = np.zeros(n_m, dtype=np.uint64), np.zeros(n_m, dtype=np.uint64), np.zeros(n_m, dtype=np.uint32)
            L.hp_paf_device_rank_members(h, k, n_m, off.ctypes.data, size.ctypes.data, crc.ctypes.data)
            out["members"].append([(int(a), int(b), int(c)) for a, b, c in zip(off, size, crc)])
        if info[1] or info[2] >= 0:
            return out
        n = int(info[3])
        cols = {f: np.zeros(n, dtype=np.uint32) for f in host.FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in host.FIELDS], cols["strand"].ctypes.data)
        out["cols"], out["slices"] = cols, [(int(slices[2 * k]), int(slices[2 * k + 1])) for k in range(world)]
        return out
    finally:
        L.hp_paf_device_free(h)


class World:
    """n_lines lines of Dataset(500, 20 000, seed)'s PAF, the same as MHAP, and the host reader's columns for both"""

    def __init__(self, tmp, n_lines, seed):
        self.dir = tmp
        self.ds = Dataset(500, 20_000, seed)
        self.names = ["r%d" % i for i in range(self.ds.n_reads)]
        self.lens = self.ds.read_len
        self.ds.write_paf(str(tmp / "all.paf"))
        with open(str(tmp / "all.paf"), "rb") as f:
            self.lines = f.read().splitlines(keepends=True)
        self.text = b"".join(self.lines[:n_lines])
        self.want = self.columns("plain", self.text)

    def columns(self, name, text, mhap=False):
        path = str(self.dir / (name + (".mhap" if mhap else ".paf")))
        with open(path, "wb") as f:
            f.write(text)
        want, bad = host.parse(path, self.names, self.lens, 2, 3 if mhap else True)
        assert bad == -1
        return want

    def write(self, name, blob, mhap=False):
        path = str(self.dir / (name + (".mhap.gz" if mhap else ".paf.gz")))
        with open(path, "wb") as f:
            f.write(blob)
        return path


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("rank_members"), 6000, 12)
    assert 200_000 < len(w.text) < 500_000
    plain = str(w.dir / "plain.paf")
    host._to_mhap(plain, str(w.dir / "as.mhap"))
    w.mhap_text = open(str(w.dir / "as.mhap"), "rb").read()
    w.want_mhap = w.columns("plain", w.mhap_text, mhap=True)
    return w


def taken(w, name, texts, blobs, n_ranks, want=None, mhap=False, options=MEMBERS):
    """the file of the members `blobs` (their texts `texts`): zlib's verdict, then the ranks' - the host reader's columns, cuts on
    run boundaries, the member list on every rank"""
    blob, text = b"".join(blobs), b"".join(texts)
    assert gm.zlib_takes(blob) == text
    r = ranks(w.write(name, blob, mhap), w.names, w.lens, n_ranks, mhap=mhap, options=options)
    print(name, "world", n_ranks, [(p["own_chunks"], p["own_jobs"], p["own_text_bytes"], p["window_markers"]) for p in r["pieces"]],
          [tuple(m[k] for k in MINFO[:5]) for m in r["members_info"]])
    assert r["irregular"] == 0 and r["bad"] == -1, (name, n_ranks, r["irregular"], r["bad"])
    gi._check_slices(r["cols"], r["slices"], (w.want_mhap if mhap else w.want) if want is None else want)
    assert all(m == listed(texts) for m in r["members"]), name
    assert sum(p["own_text_bytes"] for p in r["pieces"]) == len(text)
    assert all(m["floor_stops"] == 0 for m in r["members_info"])
    return r


def refused(w, name, blob, good, n_ranks=3, want=None, options=MEMBERS):
    """zlib refuses the file: irregular 8 on every rank with nothing set (hp_text_device_ranks checks both) and no member list,
    then the good file on the same group"""
    assert gm.zlib_takes(blob) is None, name
    r = ranks(good, w.names, w.lens, n_ranks, before=w.write(name, blob), options=options)
    assert r["was"] == (8, -1), (name, r["was"])
    assert r["irregular"] == 0 and r["bad"] == -1, name
    gi._check_slices(r["cols"], r["slices"], w.want if want is None else want)


# ---- taken -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 3, 8])
def test_two_members_cut_at_a_line_start(world, n_ranks):
    """the main case (irregular 8 before this path existed): PAF and MHAP, every rank owns jobs"""
    w = world
    for mhap, text in ((False, w.text), (True, w.mhap_text)):
        starts = line_starts(text)
        texts = cut(text, [starts[len(starts) // 2]])
        r = taken(w, "two", texts, [blocks(t) for t in texts], n_ranks, mhap=mhap)
        assert all(p["own_jobs"] > 0 and p["own_chunks"] > 0 for p in r["pieces"]), r["pieces"]
        assert sum(m["members_begun"] for m in r["members_info"]) == 2 and sum(m["member_ends"] for m in r["members_info"]) == 2
        assert sum(m["own_candidates"] for m in r["members_info"]) >= 2


def test_forty_ragged_members_from_one_line_to_100_kb(world):
    """boundaries in every rank's range, several members inside one out-window"""
    w = world
    starts = line_starts(w.text)
    rng = np.random.default_rng(4)
    big = next(s for s in starts if s >= 100_000 + starts[0])
    rest = sorted(rng.choice([s for s in starts if s > big], 37, replace=False).tolist())
    texts = cut(w.text, [starts[0], big] + rest)
    assert len(texts) == 40 and len(texts[1]) >= 100_000
    assert sum(len(t) for t in texts[-4:]) < 32768 or min(len(a) + len(b) for a, b in zip(texts[2:], texts[3:])) < 32768
    blobs = [blocks(t) for t in texts]
    # (3 and 5 ranks: over 8 a rank's text of 40 KB can lie inside the member of 100 KB, with no boundary in it)
    for n_ranks in (3, 5):
        r = taken(w, "forty", texts, blobs, n_ranks)
        assert all(m["members_begun"] + m["member_ends"] > 0 for m in r["members_info"]), r["members_info"]
        # over 5 ranks the member of 100 KB is longer than any rank's text: it spans ranks, registers travelled
        assert n_ranks < 5 or sum(m["registers_sent"] for m in r["members_info"]) >= 2


def test_twelve_cuts_in_the_middle_of_lines(world):
    w = world
    rng = np.random.default_rng(5)
    at = sorted(set(rng.integers(1, len(w.text) - 1, 12).tolist()))
    assert any(w.text[a - 1:a] != b"\n" for a in at)
    texts = cut(w.text, at)
    for n_ranks in (2, 8):
        taken(w, "midline", texts, [blocks(t) for t in texts], n_ranks)


def test_empty_members_in_front_between_and_at_the_end(world):
    w = world
    starts = line_starts(w.text)
    t = cut(w.text, [starts[100], starts[2000]])
    texts = [b"", b"", t[0], b"", t[1], b"", b"", t[2], b""]
    empties = (member(b""), member(b"", 0), dc.gz_member(b"\x03\x00", b""), dc.gz_member(b"\x01\x00\x00\xff\xff", b""))
    blobs = [blocks(x) if x else empties[k % 4] for k, x in enumerate(texts)]
    for n_ranks in (3, 8):
        taken(w, "empties", texts, blobs, n_ranks)
    taken(w, "empty_behind_one", [w.text, b""], [member(w.text), empties[2]], 3)


def test_a_rank_whose_chunks_hold_no_job(world):
    """a member of fixed codes is one job however long it is: the ranks whose chunks lie inside it own nothing, which is legal"""
    w = world
    starts = line_starts(w.text)
    texts = cut(w.text, [starts[300], starts[5500]])
    blobs = [blocks(texts[0]), member(texts[1], 6, zlib.Z_FIXED), blocks(texts[2])]
    r = taken(w, "no_job", texts, blobs, 8)
    assert any(p["own_jobs"] == 0 and p["own_chunks"] > 0 for p in r["pieces"]), r["pieces"]
    assert any(p["own_jobs"] > 0 for p in r["pieces"][1:]), r["pieces"]


def test_levels_fixed_codes_and_a_named_member(world):
    w = world
    starts = line_starts(w.text)
    n = len(starts)
    texts = cut(w.text, [starts[n * k // 6] for k in range(1, 6)])
    blobs = [member(texts[0], 0), member(texts[1], 1), member(texts[2], 6), member(texts[3], 9), member(texts[4], 6, zlib.Z_FIXED),
             member(texts[5], 6, name=b"part5.paf")]
    for n_ranks in (2, 8):
        taken(w, "levels", texts, blobs, n_ranks)


def test_one_member_with_the_option_equals_the_single_member_result(world):
    w = world
    path = w.write("one", blocks(w.text))
    with_option = ranks(path, w.names, w.lens, 3)
    without = ranks(path, w.names, w.lens, 3, options=rg.TOGETHER)
    for r in (with_option, without):
        assert r["irregular"] == 0 and r["bad"] == -1
        gi._check_slices(r["cols"], r["slices"], w.want)
    assert with_option["slices"] == without["slices"]
    for a, b in zip(with_option["pieces"], without["pieces"]):
        assert all(a[k] == b[k] for k in ("own_chunks", "own_jobs", "halo_jobs", "own_text_bytes", "window_markers", "longest_chase")), (a, b)
    assert all(m == listed([w.text]) for m in with_option["members"]) and all(m == [] for m in without["members"])
    # the one member spans all three ranks: every rank gave one register
    assert all(m["registers_sent"] == 1 for m in with_option["members_info"]), with_option["members_info"]


def edge_of(file_n, deflate_off=10):
    """the first byte of rank 1's first chunk, two ranks"""
    n_chunks = (file_n - 8 - deflate_off + CHUNK - 1) // CHUNK
    return deflate_off + CHUNK * max(1, n_chunks // 2)


def test_next_header_at_24_offsets_around_the_edge_between_two_ranks(tmp_path_factory):
    """a stored member in front sized so that the second member's header begins at 24 consecutive offsets around the first byte of
    rank 1's first chunk: the first trailer, the header and the first block of the second member each straddle the ranks' edge"""
    w = World(tmp_path_factory.mktemp("rank_sweep"), 300, 12)
    second = {}

    def place(n):
        # header 10, stored block header 5, text n, trailer 8
        if n not in second:
            second[n] = member(w.text[n:], 6)
        return 23 + n, edge_of(23 + n + len(second[n]))

    lo, hi = 1, min(len(w.text) - 100, 65_000)
    assert place(lo)[0] < place(lo)[1] and place(hi)[0] > place(hi)[1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        at, edge = place(mid)
        lo, hi = (mid, hi) if at < edge else (lo, mid)
    seen = {}
    for n in range(max(1, lo - 80), lo + 80):
        at, edge = place(n)
        if -20 <= at - edge < 4:
            seen.setdefault(at - edge, n)
    assert sorted(seen) == list(range(-20, 4)), sorted(seen)
    for d, n in sorted(seen.items()):
        texts = [w.text[:n], w.text[n:]]
        blobs = [member(texts[0], 0), second[n]]
        assert len(blobs[0]) == edge_of(len(blobs[0]) + len(blobs[1])) + d
        taken(w, "sweep", texts, blobs, 2)
    for d in (-20, -13, -8, -3, 0, 3):               # ... and the second member stored or fixed as well
        n = seen[d]
        texts = [w.text[:n], w.text[n:]]
        for tail in (member(texts[1], 0), member(texts[1], 6, zlib.Z_FIXED)):
            taken(w, "sweep_other", texts, [member(texts[0], 0), tail], 2)


# ---- the floor -----------------------------------------------------------------------------------------------------------------
def test_a_match_that_reaches_into_the_member_in_front_on_the_rank_in_front_is_refused(tmp_path_factory):
    """test_gpu_gzip_members' crafted member - 2 KB in a stored block, then a dynamic block whose first match has distance 4000,
    1952 bytes into the text of the member in front, its trailer right for the text a decoder that followed the match would give
    - placed so that the edge between the two ranks falls inside the stored block: the job that holds the match is rank 1's,
    the bytes it reaches lie in rank 0's text, and they reach rank 1 through the window in front of its piece.  zlib refuses the
    member, so flag 8 on every rank; the same blocks with the match's distance kept inside its own member are taken."""
    w = World(tmp_path_factory.mktemp("rank_floor"), 3000, 13)
    lines = w.lines
    tail = b"".join(lines[:400])
    # 2048 bytes of two lines with a tag each, the second one left open 6 bytes and a newline before its end
    l1 = lines[500][:-1] + b"\ttg:Z:" + b"A" * (1017 - len(lines[500]) - 6) + b"\n"
    l2 = lines[501][:-1] + b"\ttg:Z:"
    stored = l1 + l2 + b"B" * (2048 - len(l1) - len(l2))
    assert len(stored) == 2048 and l1[-7:] == b"AAAAAA\n"
    inside = 2048 - (len(l1) - 7)                   # the distance from the first byte behind the stored block to l1's last 7 bytes
    toks = dc.tokenise(tail)

    def crafted(dist, before):
        wr = dc.Writer()
        wr.stored(stored)
        wr.dynamic([(7, dist)] + toks[:2000])
        wr.dynamic(toks[2000:], final=True)
        text = stored + (before + stored)[len(before) + 2048 - dist:][:7] + tail
        return wr.getvalue(), text

    # the member in front grows until the ranks' edge falls inside the stored block of the crafted member behind it
    placed = None
    for n_head in range(150, 1500, 5):
        head = b"".join(lines[600:600 + n_head])
        first = member(head)
        body, would_be = crafted(4000, head)
        blob = first + dc.gz_member(body, would_be)
        d0 = len(first) + 10                        # the crafted member's deflate bytes; its dynamic block begins 2053 bytes on
        edge = edge_of(len(blob))
        if d0 + 5 + 64 <= edge <= d0 + 2053 - CHUNK // 2:
            placed = (head, first, body, would_be, blob)
            break
    assert placed, "no member in front puts the ranks' edge inside the stored block"
    head, first, body, would_be, blob = placed
    assert would_be[2048:2055] == head[len(head) - 1952:][:7]
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(body)
    assert zlib.decompressobj(-15, zdict=head[-32768:]).decompress(body) == would_be
    ok_body, ok_text = crafted(inside, head)
    assert ok_text[2048:2055] == b"AAAAAA\n" and zlib.decompressobj(-15).decompress(ok_body) == ok_text
    good_texts = [head, ok_text]
    good = w.write("reach_inside", first + dc.gz_member(ok_body, ok_text))
    want = w.columns("reach_inside", head + ok_text)
    r = taken(w, "reach_inside", good_texts, [first, dc.gz_member(ok_body, ok_text)], 2, want=want)
    # rank 1 owns jobs of the crafted member and begins inside it: it resolved symbols through a masked window
    assert r["pieces"][1]["own_jobs"] > 0 and r["members_info"][0]["members_begun"] == 2, (r["pieces"], r["members_info"])
    assert r["pieces"][0]["own_text_bytes"] > len(head)
    refused(w, "reach", blob, good, n_ranks=2, want=want)
    bad = ranks(w.write("reach", blob), w.names, w.lens, 2)
    assert bad["irregular"] == 8 and bad["cols"] is None and all(m == [] for m in bad["members"])
    print("reach", bad["pieces"], bad["members_info"])
    # rank 1's chases of the 7 copied symbols - as own symbols and as entries of its out-window - ended at the member's floor, which
    # lies in the window in front of its piece: the one rule gzip_window_compose_members_kernel adds
    assert bad["members_info"][1]["floor_stops"] >= 7 and bad["members_info"][0]["floor_stops"] == 0, bad["members_info"]


# ---- refused -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good3(world):
    w = world
    starts = line_starts(w.text)
    texts = cut(w.text, [starts[1800], starts[3900]])
    m = [blocks(t) for t in texts]
    return dict(texts=texts, m=m, blob=b"".join(m), path=w.write("good3", b"".join(m)))


def test_refusals_are_irregular_8_on_every_rank_and_the_group_goes_on(world, good3):
    w, g = world, good3
    m, good = g["m"], g["blob"]
    n = len(good)
    taken(w, "good3", g["texts"], m, 3)
    o1, o2 = len(m[0]), len(m[0]) + len(m[1])
    cases = {}
    for k in range(3):                                          # a flipped byte inside each rank's range of the file
        b = bytearray(good)
        at = 10 + (n - 18) * (2 * k + 1) // 6
        assert not (o1 - 8 <= at < o1 + 10 or o2 - 8 <= at < o2 + 10)
        b[at] ^= 0x20
        cases["flip%d" % k] = bytes(b)
    for name, at in (("crc_first", o1 - 8), ("crc_middle", o2 - 8), ("crc_last", n - 8)):
        b = bytearray(good)
        b[at] ^= 1
        cases[name] = bytes(b)
    b = bytearray(good)
    struct.pack_into("<I", b, o2 - 4, len(g["texts"][1]) + 1)
    cases["isize_middle"] = bytes(b)
    cases["isize_last"] = good[:-4] + struct.pack("<I", len(g["texts"][2]) + 1)
    cases["between"] = m[0] + b"junk" + m[1] + m[2]
    cases["zero_between"] = m[0] + b"\x00" + m[1] + m[2]
    cases["cut_last"] = good[:o2 + len(m[2]) * 2 // 3]
    cases["cut_in_header"] = m[0] + m[1] + m[2][:6]
    cases["behind"] = good + b"trailing bytes\n"
    for name, blob in cases.items():
        refused(w, name, blob, g["path"])
    # BGZF with these options alone: refused, and not taken as the text it is not
    path = str(w.dir / "bgzf.paf.gz")
    rc.write_members(w.text, path, [20_000])
    r = ranks(g["path"], w.names, w.lens, 3, before=path)
    assert r["was"] == (8, -1) and r["irregular"] == 0
    gi._check_slices(r["cols"], r["slices"], w.want)


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("rank_crafted"), 900, 13)
    w.head = b"".join(w.lines[-500:])
    w.tail, _ = dc.tagged(b"".join(w.lines[:900]))
    w.first = member(w.head)
    w.good_text = w.head + w.tail
    w.good = w.write("good", w.first + blocks(w.tail))
    w.want = w.columns("good", w.good_text)
    return w


@pytest.mark.parametrize("name", dc.INVALID_NAMES)
def test_crafted_invalid_streams_as_the_second_member(crafted, name):
    """every "invalid" stream of tests/deflate_craft.py behind an ordinary member, the change in its first and in its last block:
    what zlib refuses is irregular 8 on every rank and the group goes on; what zlib takes must give the host reader's columns"""
    w = crafted
    for place in dc.PLACES:
        body, _, got = dc.invalid(name, w.tail, place)
        blob = w.first + dc.gz_member(body, got)
        if gm.zlib_takes(blob) is None:
            refused(w, "bad_%s_%s" % (name, place), blob, w.good)
        else:
            text = gm.zlib_takes(blob)
            taken(w, "ok_%s_%s" % (name, place), [w.head, text[len(w.head):]], [w.first, dc.gz_member(body, got)], 3,
                  want=w.columns("ok_%s_%s" % (name, place), text))


def test_options_off_are_refused_as_before(world, good3):
    """without gzip_members a second member is irregular 8, without gzip_in_pieces any gzip file that is not BGZF is: as before"""
    w, g = world, good3
    for options in (rg.TOGETHER, dict(rg.TOGETHER, gzip_members=0), dict(bgzf_in_pieces=1, gzip_on_device=1, gzip_members=1, gzip_chunk_bytes=CHUNK),
                    dict(bgzf_in_pieces=1, gzip_on_device=1, gzip_in_pieces=0, gzip_members=1), dict(bgzf_in_pieces=1, gzip_in_pieces=1, gzip_members=1)):
        r = ranks(g["path"], w.names, w.lens, 3, options=options)
        assert r["cols"] is None and r["irregular"] == 8 and r["bad"] == -1, (options, r["irregular"])
        assert all(m == [] for m in r["members"]), options
        assert all(m["own_candidates"] == 0 and m["registers_sent"] == 0 for m in r["members_info"])


def test_ranks_that_disagree_on_gzip_members_all_get_einval_and_the_group_goes_on(world, good3):
    """the roll call compares the option: one rank of three with gzip_members 0 cannot make the others wait in exchanges it does
    not make - every rank's call returns RALA_HIP_EINVAL; with the option the same everywhere the same group takes the file"""
    w, g = world, good3
    for odd in (0, 1, 2):
        r = ranks(g["path"], w.names, w.lens, 3, before=g["path"], options=dict(MEMBERS, **{"gzip_members@%d" % odd: 0}))
        assert r["before_rc"] == [-2, -2, -2], r["before_rc"]   # (RALA_HIP_EINVAL on every rank)
        assert r["irregular"] == 0 and r["bad"] == -1
        gi._check_slices(r["cols"], r["slices"], w.want)
