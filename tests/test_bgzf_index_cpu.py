"""CPU: the member index of a BGZF file (rala_hip_bgzf_index, rala_amd/csrc/ingest_formats.h) - the scan for member headers block by
block and the walk of the chain from offset 0 that the device ingest builds before it ships and inflates - against a walk in
Python, and what it refuses: exactly what the host reader's BgzfSource (rala_amd/host/io.cpp) refuses."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from rala_amd import build

LIB = None


def _lib():
    global LIB
    if LIB is None:
        LIB = ctypes.CDLL(build.build_hip())
        LIB.rala_hip_bgzf_index.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 6
    return LIB


def device_index(data, block=0):
    """-> None (not BGZF) or (file offsets, compressed sizes, text sizes, text offsets)"""
    L = _lib()
    n, valid = ctypes.c_uint64(0), ctypes.c_int(0)
    assert L.rala_hip_bgzf_index(data, len(data), block, 0, ctypes.byref(n), None, None, None, None, ctypes.byref(valid)) == 0
    if not valid.value:
        return None
    m = n.value
    off, comp, text, toff = (np.zeros(m, np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint64))
    assert L.rala_hip_bgzf_index(data, len(data), block, m, ctypes.byref(n), off.ctypes.data, comp.ctypes.data, text.ctypes.data,
                                 toff.ctypes.data, ctypes.byref(valid)) == 0
    assert valid.value == 1 and n.value == m
    return off, comp, text, toff


def member(data, level=1, extra=b"", strategy=zlib.Z_DEFAULT_STRATEGY):
    """one BGZF member (as tests/test_ingest_cpu.py::_write_bgzf writes them; `extra`: another subfield in front of BC)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body = c.compress(data) + c.flush()
    xlen = len(extra) + 6
    total = 12 + xlen + len(body) + 8
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", xlen) + extra + b"BC" + struct.pack("<HH", 2, total - 1) +
            body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


EOF_MEMBER = member(b"")


def python_walk(data):
    off, comp, text, toff = [], [], [], []
    o, t = 0, 0
    while o < len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        k, bsize = 0, 0
        while k + 4 <= xlen:
            slen = struct.unpack_from("<H", data, o + 12 + k + 2)[0]
            if data[o + 12 + k:o + 14 + k] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", data, o + 12 + k + 4)[0] + 1
            k += 4 + slen
        isize = struct.unpack_from("<I", data, o + bsize - 4)[0]
        off.append(o), comp.append(bsize), text.append(isize), toff.append(t)
        o += bsize
        t += isize
    return off, comp, text, toff


def text_of(rng, n):
    words = [b"r%d" % rng.integers(0, 1 << 20) for _ in range(64)]
    out = bytearray()
    while len(out) < n:
        out += b"\t".join(words[i] for i in rng.integers(0, 64, 12)) + b"\n"
    return bytes(out[:n])


def check(data, block=0):
    got = device_index(data, block)
    assert got is not None
    want = python_walk(data)
    for g, w in zip(got, want):
        assert g.tolist() == list(w)
    return got


@pytest.mark.parametrize("seed", range(4))
def test_random_member_sizes_against_python_walk(seed):
    rng = np.random.default_rng(seed)
    text = text_of(rng, 1_500_000)
    parts, i = [], 0
    while i < len(text):
        k = int(rng.integers(1, 65537))
        parts.append(member(text[i:i + k], level=int(rng.choice([0, 1, 6, 9]))))
        i += k
    with_eof = b"".join(parts) + EOF_MEMBER
    for data in (with_eof, b"".join(parts)):
        off, comp, tsz, toff = check(data)
        assert int(tsz.sum()) == len(text)
        # the same from scans in small blocks: members across the scanner's block edges
        for block in (4096, 65536 + 3, 1 << 20):
            got = device_index(data, block)
            assert all((a == b).all() for a, b in zip(got, (off, comp, tsz, toff)))


def test_full_members_empty_members_and_extra_subfields():
    rng = np.random.default_rng(7)
    text = text_of(rng, 65536 * 3)
    data = (member(text[:65536]) + EOF_MEMBER + member(text[65536:131072], extra=b"XY" + struct.pack("<H", 5) + b"hello") + EOF_MEMBER +
            EOF_MEMBER + member(text[131072:], level=9) + EOF_MEMBER)
    off, comp, tsz, toff = check(data, block=1000)
    assert tsz.tolist() == [65536, 0, 65536, 0, 0, 65536, 0]
    # an extra subfield in the FIRST header: not what the host reader's is_bgzf recognises
    assert device_index(member(text[:1000], extra=b"XY\x00\x00") + EOF_MEMBER) is None


def test_fake_member_headers_inside_stored_blocks():
    """stored (level 0) payloads that hold whole member headers and gzip magic are not members: the walk does not stop there"""
    fake = member(b"a fake member\n")
    text = (b"x" * 100 + fake + b"\x1f\x8b\x08\x04" * 50 + fake * 20) * 200
    data = b"".join(member(text[i:i + 30000], level=0) for i in range(0, len(text), 30000)) + EOF_MEMBER
    for block in (0, 777, 4096):
        off, comp, tsz, toff = check(data, block)
        assert len(off) == (len(text) + 29999) // 30000 + 1


def test_broken_files_are_refused():
    rng = np.random.default_rng(3)
    text = text_of(rng, 300_000)
    good = b"".join(member(text[i:i + 50000]) for i in range(0, len(text), 50000)) + EOF_MEMBER
    assert device_index(good) is not None
    assert device_index(good[:-1]) is None                               # cut inside the last member
    assert device_index(good[:len(good) - len(EOF_MEMBER) - 9]) is None  # cut inside a member's trailer
    assert device_index(good[:30]) is None                               # cut inside the first member
    assert device_index(good + b"\n") is None                            # trailing garbage
    assert device_index(good + b"garbage after the members") is None
    assert device_index(good + EOF_MEMBER[:10]) is None                  # a header cut short
    assert device_index(zlib.compress(text) + b"") is None               # zlib stream, no gzip
    g = zlib.compressobj(6, zlib.DEFLATED, 31)
    assert device_index(g.compress(text) + g.flush()) is None            # plain single-member gzip
    assert device_index(text) is None                                    # plain text
    assert device_index(b"") is None
    big = bytearray(good)
    struct.pack_into("<I", big, len(member(text[:50000])) - 4, 65537)   # ISIZE > 65536
    assert device_index(bytes(big)) is None
    small = bytearray(good)
    struct.pack_into("<H", small, 16, 12 + 6 + 8 - 2)                   # BSIZE smaller than header + trailer
    assert device_index(bytes(small)) is None
