"""CPU: rala_hip_gzip_head - the RFC 1952 member header as the device ingest reads it before a single-member gzip file is
shipped: every optional field alone and all together, the deflate offset checked against where a raw inflate succeeds; what
is no such header is refused.  Headers are written here byte by byte."""
import ctypes
import gzip
import struct
import zlib

import pytest

TEXT = b"r1\t1000\t0\t900\t+\tr2\t1200\t100\t1000\t850\t900\t255\n" * 40
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def raw_deflate(data=TEXT):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def header(flg=0, extra=b"", name=b"", comment=b"", cm=8, magic=b"\x1f\x8b"):
    h = magic + bytes([cm, flg]) + struct.pack("<IBB", 0, 0, 255)
    if flg & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += name + b"\x00"
    if flg & FCOMMENT:
        h += comment + b"\x00"
    if flg & FHCRC:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def member(h, data=TEXT):
    return h + raw_deflate(data) + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def head(data):
    from rala_amd import hip

    L = hip.lib()
    off, valid = ctypes.c_uint64(77), ctypes.c_int(-1)
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    assert L.rala_hip_gzip_head(ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.byref(off), ctypes.byref(valid)) == 0
    assert valid.value in (0, 1)
    return off.value if valid.value else None


EXTRA = b"XY" + struct.pack("<H", 5) + b"hello"        # a subfield that is not BGZF's "BC"
HEADERS = {
    "none": header(),
    "text_flag": header(FTEXT),
    "name": header(FNAME, name=b"ovl.paf"),
    "extra": header(FEXTRA, extra=EXTRA),
    "empty_extra": header(FEXTRA),
    "comment": header(FCOMMENT, comment=b"made by a test"),
    "hcrc": header(FHCRC),
    "all": header(FTEXT | FHCRC | FEXTRA | FNAME | FCOMMENT, extra=EXTRA, name=b"ovl.paf", comment=b"c"),
}


@pytest.mark.parametrize("which", sorted(HEADERS))
def test_headers_with_optional_fields(which):
    h = HEADERS[which]
    data = member(h)
    assert gzip.decompress(data) == TEXT                # (the header written here is one gzip takes)
    off = head(data)
    assert off == len(h)
    d = zlib.decompressobj(-15)
    assert d.decompress(data[off:]) == TEXT and d.eof and len(d.unused_data) == 8
    # every other offset near it is not where the deflate bytes begin
    for other in (off - 1, off + 1):
        try:
            d = zlib.decompressobj(-15)
            ok = d.decompress(data[other:]) == TEXT and d.eof
        except zlib.error:
            ok = False
        assert not ok


def test_what_gzip_itself_writes(tmp_path):
    p = str(tmp_path / "ovl.paf.gz")
    with gzip.open(p, "wb") as f:
        f.write(TEXT)
    data = open(p, "rb").read()
    assert data[3] & FNAME
    off = head(data)
    assert off is not None
    assert zlib.decompressobj(-15).decompress(data[off:]) == TEXT
    data = gzip.compress(TEXT)
    assert head(data) == 10


def test_refused_headers():
    good = member(header())
    assert head(good) == 10
    assert head(b"\x1f\x8c" + good[2:]) is None             # wrong magic
    assert head(b"\x1e\x8b" + good[2:]) is None
    assert head(member(header(cm=7))) is None               # CM != 8
    for bit in (0x20, 0x40, 0x80):                          # reserved flag bits
        assert head(member(header(bit))) is None
    assert head(zlib.compress(TEXT)) is None                # a zlib stream
    assert head(TEXT) is None
    assert head(b"") is None
    assert head(good[:9]) is None
    # a header cut inside each optional field
    full = HEADERS["all"]
    assert head(full) == len(full)
    for n in range(10, len(full)):
        assert head(full[:n]) is None, n
    for which in ("name", "extra", "comment", "hcrc"):
        h = HEADERS[which]
        for n in range(10, len(h)):
            assert head(h[:n]) is None, (which, n)
