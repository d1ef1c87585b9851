"""CPU: a BGZF file in pieces by compressed byte range (rala_hip_bgzf_index_range, rala_hip_bgzf_pieces_chain;
rala_amd/csrc/ingest_formats.h) - what a rank of a sharded run makes of its share of the file without a look at the bytes in
front of it - against a walk in Python: every piece of every split, range ends on every byte of a header and a trailer, and
what the pieces refuse, for which rala_hip_bgzf_index over the whole file is the oracle."""
import ctypes
import struct

import numpy as np
import pytest

import test_bgzf_index_cpu as whole
from test_bgzf_index_cpu import EOF_MEMBER, member, text_of

LIB = None


def _lib():
    global LIB
    if LIB is None:
        LIB = whole._lib()
        LIB.rala_hip_bgzf_index_range.argtypes = [ctypes.c_char_p] + [ctypes.c_uint64] * 5 + [ctypes.c_void_p] * 8
        LIB.rala_hip_bgzf_pieces_chain.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]
    return LIB


def split(F, P, k):
    return F // P * k + min(k, F % P)


def device_piece(data, lo, hi, block=0):
    """-> (valid, begin, end, empty, [(offset, compressed size, text size)])"""
    L = _lib()
    n, valid, empty = ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_int(0)
    begin, end = ctypes.c_uint64(0), ctypes.c_uint64(0)
    tail = [ctypes.byref(begin), ctypes.byref(end), ctypes.byref(empty), ctypes.byref(valid)]
    assert L.rala_hip_bgzf_index_range(data, len(data), lo, hi, block, 0, ctypes.byref(n), None, None, None, *tail) == 0
    m = n.value
    off, comp, text = np.zeros(m, np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    if valid.value:
        assert L.rala_hip_bgzf_index_range(data, len(data), lo, hi, block, m, ctypes.byref(n), off.ctypes.data, comp.ctypes.data,
                                           text.ctypes.data, *tail) == 0
        assert n.value == m
    return bool(valid.value), begin.value, end.value, bool(empty.value), list(zip(off.tolist(), comp.tolist(), text.tolist()))


def chain(pieces, F):
    L = _lib()
    b = np.array([p[1] for p in pieces], np.uint64)
    e = np.array([p[2] for p in pieces], np.uint64)
    m = np.array([p[3] for p in pieces], np.int32)
    return L.rala_hip_bgzf_pieces_chain(b.ctypes.data, e.ctypes.data, m.ctypes.data, len(pieces), F) == 1


def is_candidate(data, q):
    return q + 12 <= len(data) and data[q:q + 3] == b"\x1f\x8b\x08" and (data[q + 3] & 4) != 0


def bsize_at(data, o):
    """what the host reader makes of the header at o: BSIZE + 1, or 0"""
    xlen = struct.unpack_from("<H", data, o + 10)[0]
    if o + 12 + xlen > len(data):
        return 0
    k, bsize = 0, 0
    while k + 4 <= xlen:
        slen = struct.unpack_from("<H", data, o + 12 + k + 2)[0]
        if data[o + 12 + k:o + 14 + k] == b"BC" and slen == 2 and k + 6 <= xlen:
            bsize = struct.unpack_from("<H", data, o + 12 + k + 4)[0] + 1
        k += 4 + slen
    return bsize if bsize >= 12 + xlen + 8 else 0


def python_piece(data, lo, hi):
    """the rule in Python: the first candidate in [lo, hi), the chain from it to an offset >= hi"""
    F = len(data)
    hi = min(hi, F)
    lo = min(lo, hi)
    q = data.find(b"\x1f\x8b\x08", lo, min(hi + 2, F))
    while q != -1 and q < hi and not is_candidate(data, q):
        q = data.find(b"\x1f\x8b\x08", q + 1, min(hi + 2, F))
    if q == -1 or q >= hi:
        return True, lo, lo, True, []
    members, o = [], q
    while o < hi:
        if not is_candidate(data, o):
            return False, q, o, False, []
        b = bsize_at(data, o)
        if b == 0 or o + b > F:
            return False, q, o, False, []
        members.append((o, b, struct.unpack_from("<I", data, o + b - 4)[0]))
        o += b
    ok = (o == F or is_candidate(data, o)) and all(m[2] <= 65536 for m in members)
    return ok, q, o, False, members if ok else []


def true_members(data):
    off, comp, text, _ = whole.python_walk(data)
    return list(zip(off, comp, text))


def make_file(rng, n_members, eof=True):
    sizes = [int(rng.choice([0, 1, 2, 100, 65536, int(rng.integers(0, 65537))])) for _ in range(n_members)]
    text = text_of(rng, sum(sizes) + 1)
    parts, at = [], 0
    for i, n in enumerate(sizes):
        extra = b"XY" + struct.pack("<H", 5) + b"hello" if i and rng.random() < 0.3 else b""
        level = int(rng.choice([1, 6] if n > 65000 else [0, 1, 6]))       # (a full member must still fit 65536 bytes)
        parts.append(member(text[at:at + n], level=level, extra=extra))
        at += n
    return b"".join(parts) + (EOF_MEMBER if eof else b"")


def check_split(data, P, block=0):
    """every piece of the split is what the walk in Python gives; returns the pieces"""
    F = len(data)
    pieces = []
    for k in range(P):
        lo, hi = split(F, P, k), split(F, P, k + 1)
        got = device_piece(data, lo, hi, block)
        want = python_piece(data, lo, hi)
        assert got[0] == want[0], (P, k, got[:4], want[:4])
        if got[0]:
            assert got == want, (P, k, got[:4], want[:4])
        pieces.append(got)
    return pieces


@pytest.mark.parametrize("n_members", [1, 2, 3, 5, 9, 17, 40])
def test_every_piece_of_every_split(n_members):
    rng = np.random.default_rng(100 + n_members)
    for eof in (True, False):
        data = make_file(rng, n_members, eof)
        truth = true_members(data)
        assert whole.device_index(data) is not None
        for P in range(1, 10):
            for block in ((0, 64, 1000) if len(data) < 300_000 else (0, 4097)):
                pieces = check_split(data, P, block)
                assert all(p[0] for p in pieces)
                assert [m for p in pieces for m in p[4]] == truth, (P, block)
                assert chain(pieces, len(data))
                # every piece holds exactly the members whose header begins in its range
                for k, p in enumerate(pieces):
                    lo, hi = split(len(data), P, k), split(len(data), P, k + 1)
                    assert p[4] == [m for m in truth if lo <= m[0] < hi]
                    assert p[3] == (not p[4])
                    if p[4]:
                        assert p[1] == p[4][0][0] and p[2] == p[4][-1][0] + p[4][-1][1]


def test_contiguity_accepts_exactly_chains():
    F = 1000
    ok = [(True, 0, 400, False), (True, 400, 400, True), (True, 400, 1000, False), (True, 1000, 1000, True)]
    assert chain(ok, F)
    assert chain([(True, 0, 1000, False)], F)
    assert not chain([(True, 0, 0, True)], F)                                             # piece 0 must hold a member
    assert not chain([(True, 0, 0, True), (True, 0, 1000, False)], F)
    assert not chain([(True, 1, 1000, False)], F)                                         # ... at offset 0
    assert not chain([(True, 0, 400, False), (True, 401, 1000, False)], F)                # a gap
    assert not chain([(True, 0, 400, False), (True, 399, 1000, False)], F)                # an overlap
    assert not chain([(True, 0, 400, False), (True, 400, 999, False)], F)                 # short of the end
    assert not chain([(True, 0, 400, False), (True, 400, 1001, False)], F)                # beyond it
    assert not chain(ok[:2], F)
    # (an empty piece's begin and end are not looked at)
    assert chain([(True, 0, 400, False), (True, 7, 3, True), (True, 400, 1000, False)], F)


def test_range_ends_on_every_byte_of_a_header_and_a_trailer():
    rng = np.random.default_rng(5)
    text = text_of(rng, 5000)
    m = [member(text[:1000]), member(text[1000:3000], extra=b"XY" + struct.pack("<H", 3) + b"abc"), member(b""), member(text[3000:]), EOF_MEMBER]
    data = b"".join(m)
    truth = true_members(data)
    F = len(data)
    at2 = len(m[0]) + len(m[1])
    # a cut at every byte from the first member's trailer to the fourth member's first deflate bytes: headers (one with an
    # extra subfield), trailers, an empty member between two cuts
    for cut in range(len(m[0]) - 10, at2 + len(m[2]) + 30):
        a, b = device_piece(data, 0, cut, 64), device_piece(data, cut, F, 64)
        assert a[0] and b[0]
        assert a[4] + b[4] == truth
        assert a[4] == [x for x in truth if x[0] < cut]
        assert chain([a, b], F)
        assert a == python_piece(data, 0, cut) and b == python_piece(data, cut, F)
    # ranges with no header start, more pieces than members
    for P in (7, 9, 50, 200):
        pieces = check_split(data, P, 64)
        assert [x for p in pieces for x in p[4]] == truth and chain(pieces, F)
        assert sum(p[3] for p in pieces) >= P - len(truth)
    inside = device_piece(data, 30, 200)
    assert inside[0] and inside[3] and inside[4] == []
    # empty members at the front, at a range's end and at the file's end
    data = EOF_MEMBER + EOF_MEMBER + m[0] + EOF_MEMBER + m[3] + EOF_MEMBER + EOF_MEMBER
    truth = true_members(data)
    F = len(data)
    for cut in range(1, F):
        a, b = device_piece(data, 0, cut, 100), device_piece(data, cut, F, 100)
        assert a[0] and b[0] and a[4] + b[4] == truth and chain([a, b], F), cut


def test_a_file_without_the_end_marker_and_broken_files_follow_the_whole_index():
    rng = np.random.default_rng(8)
    text = text_of(rng, 200_000)
    parts = [member(text[i:i + 40000]) for i in range(0, len(text), 40000)]
    good = b"".join(parts) + EOF_MEMBER
    at = [0]
    for p in parts:
        at.append(at[-1] + len(p))
    cases = {"good": good, "no_eof": b"".join(parts)}
    b = bytearray(good)
    b[at[2] + 16] ^= 0x10                                   # a byte flipped in a BSIZE: the chain lands inside the member
    cases["bsize"] = bytes(b)
    b = bytearray(good)
    b[at[3] + 17] ^= 0x80
    cases["bsize_high"] = bytes(b)
    cases["cut"] = good[:at[4] + 1000]                       # a member cut by the file's end
    cases["cut_trailer"] = good[:len(good) - 3]
    cases["between"] = good[:at[2]] + b"bytes between members\n" + good[at[2]:]
    cases["trailing"] = good + b"\n"
    b = bytearray(good)
    struct.pack_into("<I", b, at[3] - 4, 65537)             # ISIZE > 65536
    cases["isize"] = bytes(b)
    for name, data in cases.items():
        valid = whole.device_index(data) is not None
        assert valid == (name in ("good", "no_eof")), name
        for P in range(1, 10):
            for block in (0, 64, 5000):
                F = len(data)
                pieces = [device_piece(data, split(F, P, k), split(F, P, k + 1), block) for k in range(P)]
                accepted = all(p[0] for p in pieces) and chain(pieces, F)
                assert accepted == valid, (name, P, block, [p[:4] for p in pieces])
                if valid:
                    assert [m for p in pieces for m in p[4]] == true_members(data)


def header_shaped_file():
    """a stored (level 0) member whose text holds a complete member - header, BSIZE and all - placed so that it is the first
    candidate of piece 1 of 2: valid as a whole file, and the one case the pieces may refuse"""
    rng = np.random.default_rng(9)
    fake = member(b"a member that is text\n")
    text = text_of(rng, 40000)
    first = member(text[:10000])
    # the stored member straddles the middle of the file: its header in piece 0, the fake header behind the middle
    body = text[10000:30000] + fake + text[30000:31000]
    stored = member(body, level=0)
    last = member(text[31000:])
    data = first + stored + last + EOF_MEMBER
    F = len(data)
    fake_at = len(first) + data[len(first):].find(fake)
    assert len(first) < F // 2 <= fake_at < len(first) + len(stored)
    return data, fake_at


def test_a_header_shaped_string_in_a_stored_member_is_refused_not_misread():
    data, fake_at = header_shaped_file()
    F = len(data)
    assert whole.device_index(data) is not None             # the whole file is a BGZF file
    a, b = device_piece(data, 0, F // 2), device_piece(data, F // 2, F)
    assert a[0] and a[4] == true_members(data)[:2]
    assert b[1] == fake_at                                  # the false candidate starts piece 1's chain ...
    assert not (a[0] and b[0] and chain([a, b], F))         # ... and the pieces do not join: slow, never wrong
    # one piece, or a cut in front of the stored member, takes the file
    assert chain([device_piece(data, 0, F)], F)
    cut = true_members(data)[1][0]
    a, b = device_piece(data, 0, cut), device_piece(data, cut, F)
    assert a[0] and b[0] and chain([a, b], F) and a[4] + b[4] == true_members(data)


def test_the_first_header_must_be_the_host_readers():
    text = text_of(np.random.default_rng(1), 3000)
    data = member(text[:1000], extra=b"XY\x00\x00") + member(text[1000:]) + EOF_MEMBER
    assert whole.device_index(data) is None
    assert not device_piece(data, 0, len(data))[0]
    assert not device_piece(b"plain text\n" * 10, 0, 110)[0]
    assert device_piece(b"", 0, 0)[3]
