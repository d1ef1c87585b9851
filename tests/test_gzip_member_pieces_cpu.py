"""CPU: the two host functions of a gzip file of SEVERAL members taken by the ranks of a sharded run together (options
gzip_in_pieces + gzip_members) - rala_hip_gzip_compose_windows_masked, which makes the window in front of a part and masks what
lies in front of the member the part begins in, and rala_hip_gzip_members_proof, which proves every member from what the parts
owe it.  The windows are checked against the model of tests/gzip_pieces_model.py (zlib's streams decoded with every byte's
source remembered), joined from members here; the proof against zlib.crc32 per member."""
import zlib

import numpy as np
import pytest

from rala_amd import hip

import gzip_pieces_model as model

W = model.WINDOW
NOTHING = hip.GZIP_NOTHING
NONE = 0xFFFFFFFFFFFFFFFF


# ---- the model, extended to members ----------------------------------------------------------------------------------------------
def joined(texts, level):
    """members holding `texts`, each deflated on its own -> (the whole text, src of every byte in the whole text's positions,
    [first byte of every member])"""
    text, src, floors = b"", [], []
    for t in texts:
        body = model.deflate(t, level)
        got, s = model.sources(body)
        assert got == t == zlib.decompressobj(-15).decompress(body)
        floors.append(len(text))
        src.append(np.where(s >= 0, s + len(text), -1))
        text += t
    return text, (np.concatenate(src) if src else np.zeros(0, dtype=np.int64)), floors


def floor_of(floors, sizes, a):
    """first byte of the member in which the text at `a` begins: the last member that is not empty and begins at or before a
    (behind the text's end: a itself)"""
    f = a
    for at, n in zip(floors, sizes):
        if n and at <= a < at + n:
            f = at
    return f


def reaches(floors, sizes, cuts):
    return [min(a - floor_of(floors, sizes, a), W) for a in cuts[:-1]]


def masked_window(text, a, reach):
    w = model.window_in_front(text, a, NOTHING)
    w[:W - min(reach, W)] = NOTHING
    return w


def check(text, src, floors, sizes, cuts):
    windows = model.windows_of(text, src, cuts)
    reach = reaches(floors, sizes, cuts)
    for part in range(len(cuts) - 1):
        got, before, valid = hip.gzip_compose_windows_masked(windows, reach, part)
        a = cuts[part]
        assert valid, (cuts, part)
        want = masked_window(text, a, reach[part])
        assert (got == want).all(), (cuts, part, int(np.argmax(got != want)))
        # the byte in front is the text's, whatever member it belongs to
        assert before == (text[a - 1] if a else -1), (cuts, part)
        # ... and with no member boundary within reach the unmasked composition says the same
        plain, ok = hip.gzip_compose_windows(windows, part)
        assert ok and (plain == model.window_in_front(text, a, NOTHING)).all()


@pytest.fixture(scope="module")
def base():
    return model.far_text(150_000, 5)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_members_joined_and_cut_anywhere(base, level):
    """1 - 6 members cut into 1 - 9 parts at arbitrary offsets: the window in front of a part is the text in front of it as far
    back as the member it begins in reaches, nothing in front of that"""
    rng = np.random.default_rng(level)
    n = len(base)
    for n_members in range(1, 7):
        at = [0] + sorted(int(x) for x in rng.integers(1, n, n_members - 1)) + [n]
        texts = [base[a:b] for a, b in zip(at[:-1], at[1:])]
        text, src, floors = joined(texts, level)
        sizes = [len(t) for t in texts]
        assert text == base
        for parts in sorted(set((1, 2, 3 + n_members, 9))):
            inner = sorted(int(x) for x in rng.integers(0, n + 1, parts - 1))
            check(text, src, floors, sizes, [0] + inner + [n])


def test_parts_at_and_just_behind_a_members_first_byte(base):
    """a part that begins at a member's first byte gets a window of nothing, and the byte in front is still the text's; 1 and
    32 767 bytes behind it the window holds exactly that many bytes"""
    n = len(base)
    f1, f2 = 40_000, 95_000
    texts = [base[:f1], base[f1:f2], base[f2:]]
    text, src, floors = joined(texts, 6)
    sizes = [len(t) for t in texts]
    cuts = [0, f1, f1 + 1, f2, f2 + W - 1, n]
    check(text, src, floors, sizes, cuts)
    windows = model.windows_of(text, src, cuts)
    reach = reaches(floors, sizes, cuts)
    assert reach == [0, 0, 1, 0, W - 1]
    for part, keep in ((1, 0), (2, 1), (3, 0), (4, W - 1)):
        got, before, valid = hip.gzip_compose_windows_masked(windows, reach, part)
        assert valid and (got[:W - keep] == NOTHING).all() and (got[W - keep:] < 0x100).all()
        assert before == text[cuts[part] - 1]
    # clamped: a part far behind its member's first byte has the whole window
    cuts = [0, f1 + 50_000, n]
    assert reaches(floors, sizes, cuts) == [0, W]
    check(text, src, floors, sizes, cuts)


def test_members_shorter_than_a_window_and_empty_ones_and_empty_parts(base):
    """an out-window that straddles three members; members of no text in front, between and at the end; parts of no text"""
    at = [0, 0, 9_000, 20_000, 20_000, 27_000, 31_000, 60_000, len(base), len(base)]
    texts = [base[a:b] for a, b in zip(at[:-1], at[1:])]
    text, src, floors = joined(texts, 6)
    sizes = [len(t) for t in texts]
    n = len(text)
    # the piece [5 000, 30 000) ends in the fourth member that has text: its out-window holds bytes of three members
    check(text, src, floors, sizes, [0, 5_000, 30_000, n])
    check(text, src, floors, sizes, [0, 0, 5_000, 5_000, 20_000, 20_000, 26_999, 27_000, 27_001, n])
    check(text, src, floors, sizes, [0, 31_000, 31_000, 31_000, 61_000, n, n])


def test_a_marker_that_lands_in_front_of_the_floor_finds_nothing():
    """a match of the second member that reaches 1 952 bytes into the first member's text (what zlib refuses): the unmasked window
    in front of a part that begins inside the second member holds the byte, the masked one does not - the part's resolve meets
    nothing and refuses; and a window that claims a member reached further back than there is text is not valid"""
    rng = np.random.default_rng(8)
    n, floor = 80_000, 40_000
    text = rng.integers(40, 111, n).astype(np.uint8).tobytes()
    src = np.full(n, -1, dtype=np.int64)
    at = floor + 2048
    src[at:at + 7] = np.arange(at, at + 7) - 4000              # (the model's text need not be what a decoder would write)
    a = floor + 1000
    cuts = [0, 20_000, a, n]
    windows = model.windows_of(text, src, cuts)
    entry = W - (a - (at - 4000))
    plain, ok = hip.gzip_compose_windows(windows, 2)
    assert ok and plain[entry] == text[at - 4000]
    got, before, valid = hip.gzip_compose_windows_masked(windows, [0, 20_000, 1000], 2)
    assert valid and got[entry] == NOTHING and before == text[a - 1]
    assert (got[W - 1000:] == np.frombuffer(text[a - 1000:a], dtype=np.uint8)).all() and (got[:W - 1000] == NOTHING).all()
    # the part's own symbol at `at` is the marker of that entry: through the masked window it is no byte
    own = model.out_window(text, src, a, a + W)
    assert own[at - a] == (0x8000 | entry)
    # a reach beyond the text's first byte: invalid, for the part itself and for a part in front of it
    assert hip.gzip_compose_windows_masked(windows, [0, 20_001, 1000], 1)[2] is False
    assert hip.gzip_compose_windows_masked(windows, [0, 20_001, 1000], 2)[2] is False
    assert hip.gzip_compose_windows_masked(windows, [1, 20_000, 1000], 2)[2] is False
    # what the unmasked composition refuses stays refused
    bad = windows.copy()
    bad[1, 77] = 0x0100
    assert hip.gzip_compose_windows_masked(bad, [0, 20_000, 1000], 2)[2] is False


def test_masked_composition_refuses_bad_arguments():
    import ctypes

    L = hip.lib()
    w, r = np.zeros(W, dtype=np.uint16), np.zeros(1, dtype=np.uint64)
    before, valid = ctypes.c_int32(0), ctypes.c_int32(0)
    f = L.rala_hip_gzip_compose_windows_masked
    assert f(w.ctypes.data, 1, r.ctypes.data, 1, w.ctypes.data, ctypes.byref(before), ctypes.byref(valid)) != 0
    assert f(None, 1, r.ctypes.data, 0, w.ctypes.data, ctypes.byref(before), ctypes.byref(valid)) != 0
    assert f(w.ctypes.data, 1, None, 0, w.ctypes.data, ctypes.byref(before), ctypes.byref(valid)) != 0


# ---- the proof over parts --------------------------------------------------------------------------------------------------------
def register(data):
    """the CRC register of the bytes from zero, without the final inversion (rala_hip_crc32_chain's convention)"""
    return (zlib.crc32(data) ^ zlib.crc32(bytes(len(data)))) & 0xFFFFFFFF


def owed(texts, trailers, cuts):
    """what every part [cuts[p], cuts[p + 1]) owes: (head, tail, local_bad) per part, as a rank computes them from its own text -
    head: its first bytes where they belong to a member begun in front of it; tail: its last bytes where they belong to a member
    begun in it that goes on behind it; local_bad: the first member inside its text alone whose CRC32 is not its trailer"""
    text = b"".join(texts)
    lo = np.concatenate(([0], np.cumsum([len(t) for t in texts]))).astype(int)
    head, tail, bad, names = [], [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        h, t, bd, nm = (0, 0), (0, 0), None, [None, None]
        for m, x in enumerate(texts):
            m0, m1 = int(lo[m]), int(lo[m + 1])
            if m0 == m1 or a == b:
                continue
            if m0 < a < m1:
                h, nm[0] = (register(text[a:min(b, m1)]), min(b, m1) - a), m
            elif a <= m0 < b < m1:
                t, nm[1] = (register(text[m0:b]), b - m0), m
            elif a <= m0 and m1 <= b and bd is None and zlib.crc32(x) != trailers[m]:
                bd = m
        head.append(h)
        tail.append(t)
        bad.append(bd)
        names.append(nm)
    return head, tail, bad, names


def listed(texts, trailers):
    out, at = [], 0
    for t, c in zip(texts, trailers):
        out.append((at, len(t), c))
        at += len(t)
    return out


def members_for_proof():
    rng = np.random.default_rng(21)
    sizes = [0, 1, 100_000, 0, 3_000, 1, 40_000, 17, 0, 60_000, 0]
    return [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in sizes]


CUTS = {
    "one part": [0, 203_019],
    "inside, across two, across all": [0, 50_000, 101_000, 103_500, 143_000, 150_000, 203_019],
    "a boundary on every member edge": [0, 1, 100_001, 103_001, 103_002, 143_002, 143_019, 203_019],
    "empty parts": [0, 0, 70_000, 70_000, 70_000, 160_000, 203_019, 203_019],
    "one member over nine parts": [0] + [10_000 * k + 5 for k in range(1, 9)] + [203_019],
}


def test_register_convention():
    data = b"what the chain is made of"
    regs = np.array([register(data[:7]), register(data[7:])], dtype=np.uint32)
    lens = np.array([7, len(data) - 7], dtype=np.uint64)
    L = hip.lib()
    L.rala_hip_crc32_chain.restype = np.ctypeslib.ctypes.c_uint32
    L.rala_hip_crc32_chain.argtypes = [np.ctypeslib.ctypes.c_void_p] * 2 + [np.ctypeslib.ctypes.c_uint64]
    assert L.rala_hip_crc32_chain(regs.ctypes.data, lens.ctypes.data, 2) == zlib.crc32(data)


@pytest.mark.parametrize("name", list(CUTS))
def test_every_member_is_proven_and_every_wrong_word_names_its_member(name):
    texts = members_for_proof()
    cuts = CUTS[name]
    assert cuts[-1] == sum(len(t) for t in texts)
    trailers = [zlib.crc32(t) for t in texts]
    parts = list(zip(cuts[:-1], cuts[1:]))
    head, tail, bad, names = owed(texts, trailers, cuts)
    assert bad == [None] * len(parts)
    assert hip.gzip_members_proof(listed(texts, trailers), parts, head, tail, bad) == (True, len(texts))
    spanning = set()
    for p in range(len(parts)):
        for regs, who in ((head, names[p][0]), (tail, names[p][1])):
            if who is None:
                assert regs[p] == (0, 0)
                # a register nobody owes is refused too
                wrong = list(regs)
                wrong[p] = (0, 1)
                got = hip.gzip_members_proof(listed(texts, trailers), parts, wrong if regs is head else head, wrong if regs is tail else tail, bad)
                assert got[0] is False, (name, p)
                continue
            spanning.add(who)
            for reg, n in ((regs[p][0] ^ 1, regs[p][1]), (regs[p][0], regs[p][1] + 1), (regs[p][0], regs[p][1] - 1)):
                wrong = list(regs)
                wrong[p] = (reg, n)
                got = hip.gzip_members_proof(listed(texts, trailers), parts, wrong if regs is head else head, wrong if regs is tail else tail, bad)
                assert got == (False, who), (name, p, got)
    # every trailer, one at a time: a member inside one part is caught by that part, one that spans parts by the chain
    for m, t in enumerate(texts):
        wrong = list(trailers)
        wrong[m] ^= 0x80000000
        h2, t2, bad2, _ = owed(texts, wrong, cuts)
        assert (h2, t2) == (head, tail)
        got = hip.gzip_members_proof(listed(texts, wrong), parts, head, tail, bad2)
        assert got == (False, m), (name, m, got)
        if len(t) and m not in spanning:
            assert bad2.count(m) == 1
    # the text's size must be the parts'
    short = list(parts)
    short[-1] = (short[-1][0], short[-1][1] - 1) if short[-1][1] > short[-1][0] else short[-1]
    if short != parts:
        assert hip.gzip_members_proof(listed(texts, trailers), short, head, tail, bad) == (False, len(texts))


def test_spans_of_the_cases():
    """the cases hold what they say: members inside one part, across two parts, across all parts"""
    texts = members_for_proof()
    trailers = [zlib.crc32(t) for t in texts]
    _, _, _, names = owed(texts, trailers, CUTS["inside, across two, across all"])
    across = [m for nm in names for m in nm if m is not None]
    assert across.count(2) == 2 and across.count(6) == 3 and not {1, 5, 7} & set(across)
    _, _, _, names = owed(texts, trailers, CUTS["one part"])
    assert names == [[None, None]]
    _, _, _, names = owed(texts, trailers, CUTS["one member over nine parts"])
    assert all(nm != [None, None] for nm in names)


def test_the_bench_tool_writes_members_cut_at_line_starts(tmp_path):
    """tools/ranks_gzip_members_bench.py: the file it times is a chain of gzip members that is the PAF's text, every member but the
    last ending with a line"""
    import gzip
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import ranks_gzip_members_bench as bench

    text = model.far_text(60_000, 3)
    src, dst = str(tmp_path / "ovl.paf"), str(tmp_path / "members.paf.gz")
    open(src, "wb").write(text)
    n = bench.write_members(src, dst, member_text=9_000)
    blob = open(dst, "rb").read()
    assert 5 <= n <= 7 and gzip.decompress(blob) == text
    sizes = []
    while blob:
        d = zlib.decompressobj(31)
        part = d.decompress(blob)
        # every member is whole and ends with a line; all but the last hold at least the text asked for
        assert d.eof and part.endswith(b"\n") and (len(part) >= 9_000 or not d.unused_data)
        sizes.append(len(part))
        blob = d.unused_data
    assert len(sizes) == n and sum(sizes) == len(text)
