"""GPU: gzip overlap files of SEVERAL members that are not BGZF (cat part*.paf.gz, pigz -i, a .gz file that was appended to)
inflated on the device with the options gzip_on_device and gzip_members (rala_amd/csrc/inflate_kernels.hip:
gzip_member_find_kernel, the member spans of gzip_count_kernel, the member floors of the windows / resolve kernels,
gzip_piece_crc_kernel; ingest_formats.h: gzip_chain_members).  The verdict on every file is zlib's (Python's gzip inflates each
one here) and the host reader's rule: a good file gives the plain file's columns with no flag - a fallback is a failure - and
the member list rala_hip_get_gzip_members gives is the one the test wrote; a file zlib refuses gives flag 8 and no rows.
Texts are a few hundred KB at most; chunks of 1024 compressed bytes where chunk edges matter."""
import ctypes
import gzip
import struct
import zlib

import numpy as np
import pytest

from rala_amd import hip
from rala_amd.synth import Dataset

import deflate_craft as dc
import test_gpu_gzip as gg
import test_gpu_ingest as gi

pytestmark = pytest.mark.gpu
TILE = 4096                 # bytes per workgroup of the member find


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, name=None):
    return dc.gz_member(gg.deflate(text, level=level, strategy=strategy), text, name)


def listed(texts):
    """the member list of a file whose members hold `texts`: (text offset, text size, CRC32)"""
    out, at = [], 0
    for t in texts:
        out.append((at, len(t), zlib.crc32(t) & 0xFFFFFFFF))
        at += len(t)
    return out


def device(path, w, members=1, **options):
    """the file through rala_hip_set_overlaps_from_paf with gzip_on_device, gzip_members and `options` set -> gg.device's result
    (columns or None, irregular flags, first length-check offender, the inflater's counts, rows) and the member list
    rala_hip_get_gzip_members gave behind the call"""
    L = gg._lib()
    L.hp_paf_device_gzip_members.restype = ctypes.c_uint64
    L.hp_paf_device_gzip_members.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 3
    options = dict(options, gzip_on_device=1, gzip_members=members)
    keys = (ctypes.c_char_p * len(options))(*[k.encode() for k in options])
    values = np.array(list(options.values()), dtype=np.int64)
    rl = np.ascontiguousarray(w.ds.read_len, dtype=np.uint32)
    h = L.hp_text_device_with(path.encode(), "\n".join(w.names).encode(), rl.ctypes.data, len(rl), 1, 4, 0, ctypes.cast(keys, ctypes.c_void_p),
                              values.ctypes.data, len(options))
    try:
        info, g = np.zeros(6, dtype=np.int64), np.zeros(10, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        L.hp_paf_device_gzip_info(h, g.ctypes.data)
        assert info[0] == 0, info
        gz = dict(zip(gg.GZ_KEYS, (int(x) for x in g)))
        n_m = L.hp_paf_device_gzip_members(h, 0, None, None, None)
        off, size, crc = np.zeros(n_m, dtype=np.uint64), np.zeros(n_m, dtype=np.uint64), np.zeros(n_m, dtype=np.uint32)
        L.hp_paf_device_gzip_members(h, n_m, off.ctypes.data, size.ctypes.data, crc.ctypes.data)
        members = [(int(a), int(b), int(c)) for a, b, c in zip(off, size, crc)]
        if info[1] or info[2] >= 0:
            return (None, int(info[1]), int(info[2]), gz, int(info[3])), members
        n = int(info[3])
        cols = {f: np.zeros(n, dtype=np.uint32) for f in gg.FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in gg.FIELDS], cols["strand"].ctypes.data)
        return (cols, 0, -1, gz, n), members
    finally:
        L.hp_paf_device_free(h)


def zlib_takes(blob):
    """zlib's inflate over the file member by member, nothing allowed between or behind them: the text, or None"""
    out = b""
    while blob:
        d = zlib.decompressobj(31)
        try:
            out += d.decompress(blob)
        except zlib.error:
            return None
        if not d.eof:
            return None
        blob = d.unused_data
    return out


class World:
    """n_lines lines of a data set's PAF (tagged: dc.paf_text), the plain file's columns through the device tokeniser"""

    def __init__(self, tmp, n_lines, seed, text=None):
        self.dir = tmp
        self.ds = Dataset(500, 20_000, seed)
        self.names = ["r%d" % i for i in range(self.ds.n_reads)]
        self.ds.write_paf(str(tmp / "all.paf"))
        with open(str(tmp / "all.paf"), "rb") as f:
            self.lines = f.read().splitlines(keepends=True)
        self.text = b"".join(self.lines[:n_lines]) if text is None else text(self)
        self.want = self.parse("plain", self.text)

    def parse(self, name, text):
        path = str(self.dir / (name + ".paf"))
        with open(path, "wb") as f:
            f.write(text)
        want, irregular, bad = gi.device_parse(path, self.names, self.ds.read_len)
        assert irregular == 0 and bad == -1
        return want

    def write(self, name, blob):
        path = str(self.dir / (name + ".paf.gz"))
        with open(path, "wb") as f:
            f.write(blob)
        return path


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("members"), 6000, 12)
    assert 200_000 < len(w.text) < 500_000
    return w


def accepted(w, name, texts, blobs, want=None, **options):
    """the file of the members `blobs` (their texts `texts`): zlib's verdict, then the device's"""
    blob = b"".join(blobs)
    text = b"".join(texts)
    assert gzip.decompress(blob) == text and zlib_takes(blob) == text
    (res, members) = device(w.write(name, blob), w, **options)
    print(name, options, end=" ")
    gg.good(res, w.want if want is None else want, len(text))
    assert members == listed(texts), name
    return res[3]


def cut(text, at):
    at = [0] + sorted(at) + [len(text)]
    return [text[a:b] for a, b in zip(at[:-1], at[1:])]


def line_starts(text):
    return (np.flatnonzero(np.frombuffer(text, dtype=np.uint8)[:-1] == 10) + 1).tolist()


# ---- the member find alone ---------------------------------------------------------------------------------------------------
def gzip_head_at_every_offset(buf):
    L = hip.lib()
    base = (ctypes.c_uint8 * len(buf)).from_buffer_copy(buf)
    addr = ctypes.addressof(base)
    f = L.rala_hip_gzip_head
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
    off, valid = ctypes.c_uint64(0), ctypes.c_int(0)
    out = []
    for at in range(len(buf)):
        assert f(addr + at, len(buf) - at, ctypes.byref(off), ctypes.byref(valid)) == 0
        if valid.value:
            out.append((at, at + off.value))
    return out


def header(flg, xlen=0, name=b"a name", comment=b"a comment, longer"):
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\x01\x02\x03\x04\x00\xff"
    if flg & 4:
        h += struct.pack("<H", xlen) + bytes(1 + k % 255 for k in range(xlen))
    if flg & 8:
        h += name + b"\x00"
    if flg & 16:
        h += comment + b"\x00"
    if flg & 2:
        h += b"\xaa\xbb"
    return h


def test_member_find_equals_gzip_head_at_every_offset():
    rng = np.random.default_rng(3)
    n = 256 * 1024
    buf = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    planted, at = [], 1000
    for flg in range(32):                            # FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT in every combination
        for xlen in ((0, 300) if flg & 4 else (0,)):
            h = header(flg, xlen)
            buf[at:at + len(h)] = h
            planted.append((at, at + len(h)))
            at += len(h) + 700
    assert at < 40 * 1024
    for k, d in enumerate(range(-14, 3)):           # a header at every offset across a tile edge (an edge each)
        h = header(8 | 4, 5)
        p = TILE * (12 + k) + d
        buf[p:p + len(h)] = h
        planted.append((p, p + len(h)))
    far = header(8, name=bytes(1 + k % 200 for k in range(3 * TILE)))       # a name that ends three tiles on
    buf[TILE * 40 + 7:TILE * 40 + 7 + len(far)] = far
    planted.append((TILE * 40 + 7, TILE * 40 + 7 + len(far)))
    for k, bad in enumerate((b"\x1f\x8b\x07\x00", b"\x1f\x8b\x09\x08", b"\x1f\x8b\x08\x20", b"\x1f\x8b\x08\x48", b"\x1f\x8b\x08\x80")):
        buf[TILE * 50 + 100 * k:TILE * 50 + 100 * k + 4] = bad           # CM != 8, reserved flag bits
    buf[TILE * 52:TILE * 52 + 14] = b"\x1f" + header(0)                 # 1f 1f 8b 08
    planted.append((TILE * 52 + 1, TILE * 52 + 11))
    buf[TILE * 53 - 2:TILE * 53 + 8] = header(0)                        # the magic itself across an edge
    planted.append((TILE * 53 - 2, TILE * 53 + 8))
    tail = b"\x1f\x8b\x08\x08" + b"\x00" * 4 + b"\x00\xff" + b"no end"  # a header cut by the buffer's end
    buf[n - len(tail):] = tail
    buf[n - 40:n - 36] = b"\x1f\x8b\x08\x04"                            # ... and an extra field that reaches beyond it
    buf[n - 30:n - 28] = struct.pack("<H", 500)
    want = gzip_head_at_every_offset(bytes(buf))
    assert set(planted) <= set(want) and n - len(tail) not in dict(want) and n - 40 not in dict(want)
    ctx = hip.Context(0)
    try:
        got = ctx.gzip_find_members(bytes(buf))
        assert got == want
        for cutoff in (TILE * 12 - 3, TILE * 40 + 9, 11, 10, 9, 0):     # other sizes: the last tile partial, nearly nothing, nothing
            assert ctx.gzip_find_members(bytes(buf[:cutoff])) == gzip_head_at_every_offset(bytes(buf[:cutoff])), cutoff
        assert ctx.gzip_find_members(header(0)) == [(0, 10)]
    finally:
        ctx.close()


# ---- overlap files, accepted -------------------------------------------------------------------------------------------------
def test_two_members(world):
    w = world
    starts = line_starts(w.text)
    texts = cut(w.text, [starts[len(starts) // 2]])
    for options in ({}, dict(gzip_chunk_bytes=1024), dict(gzip_chunk_bytes=1024, ingest_window_bytes=50_000)):
        accepted(w, "two", texts, [member(t) for t in texts], **options)


def test_forty_ragged_members_from_one_line_to_100_kb(world):
    w = world
    starts = line_starts(w.text)
    rng = np.random.default_rng(4)
    big = next(s for s in starts if s >= 100_000 + starts[0])
    rest = sorted(rng.choice([s for s in starts if s > big], 37, replace=False).tolist())
    texts = cut(w.text, [starts[0], big] + rest)
    assert len(texts) == 40 and len(texts[0]) == len(w.lines[0]) and len(texts[1]) >= 100_000
    for options in ({}, dict(gzip_chunk_bytes=1024)):
        accepted(w, "forty", texts, [member(t) for t in texts], **options)


def test_members_cut_in_the_middle_of_a_line(world):
    w = world
    rng = np.random.default_rng(5)
    at = sorted(set(rng.integers(1, len(w.text) - 1, 12).tolist()))
    assert any(w.text[a - 1:a] != b"\n" for a in at)
    texts = cut(w.text, at)
    accepted(w, "midline", texts, [member(t) for t in texts], gzip_chunk_bytes=1024)


def test_empty_members_in_front_between_and_at_the_end(world):
    w = world
    starts = line_starts(w.text)
    t = cut(w.text, [starts[100], starts[2000]])
    texts = [b"", b"", t[0], b"", t[1], b"", b"", t[2], b""]
    empties = (member(b""), member(b"", 0), dc.gz_member(b"\x03\x00", b""), dc.gz_member(b"\x01\x00\x00\xff\xff", b""))
    blobs = [member(x) if x else empties[k % 4] for k, x in enumerate(texts)]
    for options in ({}, dict(gzip_chunk_bytes=1024)):
        accepted(w, "empties", texts, blobs, **options)
    accepted(w, "empty_behind_one", [w.text, b""], [member(w.text), empties[2]])


def test_members_of_every_level_fixed_codes_and_a_name(world):
    w = world
    starts = line_starts(w.text)
    n = len(starts)
    texts = cut(w.text, [starts[n * k // 6] for k in range(1, 6)])
    blobs = [member(texts[0], 0), member(texts[1], 1), member(texts[2], 6), member(texts[3], 9), member(texts[4], 6, zlib.Z_FIXED),
             member(texts[5], 6, name=b"part5.paf")]
    for options in ({}, dict(gzip_chunk_bytes=1024)):
        accepted(w, "levels", texts, blobs, **options)
    # every member's first block of one kind: stored, fixed, dynamic - final or not
    for tag, level, strategy in (("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("dynamic", 9, zlib.Z_DEFAULT_STRATEGY)):
        some = cut(w.text, [starts[7], starts[9], starts[1500]])
        accepted(w, "all_" + tag, some, [member(t, level, strategy) for t in some], gzip_chunk_bytes=1024)


def test_next_header_at_24_offsets_around_a_chunk_edge(tmp_path_factory):
    """a stored member in front whose size puts the second member's header at 24 consecutive offsets around the edge between
    two chunks of 1024 bytes: the first trailer, the header and the first block of the second member each straddle it"""
    w = World(tmp_path_factory.mktemp("sweep"), 300, 12)
    edge = 10 + 3 * 1024                            # chunks are counted from the first member's deflate bytes
    for at in range(edge - 20, edge + 4):
        n = at - 23                                 # header 10, stored block header 5, text n, trailer 8
        texts = [w.text[:n], w.text[n:]]
        blobs = [member(texts[0], 0), member(texts[1], 6)]
        assert len(blobs[0]) == at
        accepted(w, "sweep", texts, blobs, gzip_chunk_bytes=1024)
    for at in range(edge - 20, edge + 4, 5):        # ... and the second member stored or fixed as well
        n = at - 23
        texts = [w.text[:n], w.text[n:]]
        accepted(w, "sweep0", texts, [member(texts[0], 0), member(texts[1], 0)], gzip_chunk_bytes=1024)
        accepted(w, "sweepf", texts, [member(texts[0], 0), member(texts[1], 6, zlib.Z_FIXED)], gzip_chunk_bytes=1024)


# ---- crafted streams as the second member ------------------------------------------------------------------------------------
class Crafted(World):
    """an ordinary member of 500 lines in front of a second member whose text is `tail`"""

    def __init__(self, tmp, n_lines, seed, marker=False):
        def text(w):
            w.head = b"".join(w.lines[-500:])
            w.tail, w.far_at = dc.tagged(b"".join(w.lines[:n_lines]))
            if marker:
                w.tail = dc.marker_text(b"".join(w.lines), n_lines)
            return w.head + w.tail
        super().__init__(tmp, n_lines, seed, text)
        self.first = member(self.head)


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    return Crafted(tmp_path_factory.mktemp("crafted"), 3000, 13)


@pytest.fixture(scope="module")
def marker(tmp_path_factory):
    return Crafted(tmp_path_factory.mktemp("marker"), 600, 12, marker=True)


@pytest.mark.parametrize("name", list(dc.VALID) + list(dc.GZIP_ONLY))
def test_valid_crafted_stream_as_the_second_member(crafted, marker, name):
    w = marker if name == "marker_copies" else crafted
    body, _ = dict(dc.VALID, **dc.GZIP_ONLY)[name](w.tail)
    assert dc.verdict(body) == w.tail
    for chunk in (1024, None):
        accepted(w, "valid_" + name, [w.head, w.tail], [w.first, dc.gz_member(body, w.tail)], **({} if chunk is None else dict(gzip_chunk_bytes=chunk)))


def refused(w, name, blob, **options):
    assert zlib_takes(blob) is None, name
    res, members = device(w.write(name, blob), w, **options)
    print(name, options, res[3])
    assert res[0] is None and res[1] & 8 and res[2] == -1 and res[4] == 0 and members == [], (name, options, res[1:])


@pytest.mark.parametrize("place", dc.PLACES)
@pytest.mark.parametrize("name", dc.INVALID_NAMES)
def test_invalid_crafted_stream_as_the_second_member_is_flag_8_and_no_rows(crafted, name, place):
    w = crafted
    body, _, got = dc.invalid(name, w.tail, place)
    assert dc.verdict(body) is None
    refused(w, "bad_%s_%s" % (name, place), w.first + dc.gz_member(body, got), gzip_chunk_bytes=4096)


def test_a_match_that_reaches_into_the_member_in_front_is_refused(crafted):
    """the second member: 2 KB of stored random bytes, then a dynamic block whose first match has distance 4000 - 1952 bytes
    into the first member's text - and a trailer computed for the text a decoder that followed it there would give.  zlib
    refuses the member (nothing lies in front of a member); a chunk that starts at the dynamic block knows nothing of the 2 KB
    in front of it, so only the member floor of the windows / resolve passes can (chunks of 1024 bytes); with one chunk for the
    whole member the counting pass sees it"""
    w = crafted
    rng = np.random.default_rng(8)
    stored = rng.integers(40, 111, 2048).astype(np.uint8).tobytes()
    toks = dc.tokenise(w.tail[:60_000])
    reach = w.head[len(w.head) + 2048 - 4000:][:7]
    assert len(reach) == 7
    wr = dc.Writer()
    wr.stored(stored)
    wr.dynamic([(7, 4000)] + toks[:4000])
    wr.dynamic(toks[4000:], final=True)
    body = wr.getvalue()
    would_be = stored + reach + w.tail[:60_000]
    d = zlib.decompressobj(-15)
    with pytest.raises(zlib.error):
        d.decompress(body)
    # the same blocks behind the first member's text in ONE stream are valid, and give that text: only the member boundary is wrong
    whole = zlib.decompressobj(-15, zdict=w.head[-32768:])
    assert whole.decompress(body) == would_be
    blob = w.first + dc.gz_member(body, would_be)
    for options in (dict(gzip_chunk_bytes=1024), {}):
        refused(w, "reach", blob, **options)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_a_good_file_behind_them_on_the_same_context(world):
    w = world
    starts = line_starts(w.text)
    texts = cut(w.text, [starts[800], starts[1700]])
    m = [member(t) for t in texts]
    good = b"".join(m)
    accepted(w, "good3", texts, m, gzip_chunk_bytes=4096)
    o1, o2 = len(m[0]), len(m[0]) + len(m[1])
    cases = {}
    b = bytearray(good)
    b[o1 + len(m[1]) // 2] ^= 0x55
    cases["flipped byte in member 2"] = bytes(b)
    b = bytearray(good)
    b[o2 - 8] ^= 1
    cases["crc of the middle member"] = bytes(b)
    b = bytearray(good)
    struct.pack_into("<I", b, o2 - 4, len(texts[1]) + 1)
    cases["isize of the middle member"] = bytes(b)
    b = bytearray(good)
    b[o1 - 8:o1 - 4], b[o2 - 8:o2 - 4] = good[o2 - 8:o2 - 4], good[o1 - 8:o1 - 4]
    cases["crcs of two members exchanged"] = bytes(b)
    cases["bytes behind the last trailer"] = good + b"trailing bytes\n"
    cases["bytes between two members"] = m[0] + b"junk" + m[1] + m[2]
    cases["a zero byte between two members"] = m[0] + b"\x00" + m[1] + m[2]
    cases["a cut inside the second header"] = m[0] + m[1][:6]
    cases["a cut inside the second member"] = m[0] + m[1][:len(m[1]) // 2]
    cases["a second header with a reserved flag bit"] = m[0] + m[1][:3] + b"\x20" + m[1][4:] + m[2]
    for name, blob in cases.items():
        for chunk in (4096, 1 << 20):
            refused(w, name.replace(" ", "_"), blob, gzip_chunk_bytes=chunk)
    # with gzip_members 0 a file of several members is refused as it ever was
    res, members = device(w.write("off", good), w, members=0, gzip_chunk_bytes=4096)
    assert res[0] is None and res[1] & 8 and res[4] == 0 and members == []
    # one context: a refused file, then the good one
    L = gg._lib()
    L.hp_text_device_after.restype = ctypes.c_void_p
    L.hp_text_device_after.argtypes = [ctypes.c_char_p] + list(L.hp_text_device_with.argtypes)
    L.hp_paf_device_before.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    options = dict(gzip_on_device=1, gzip_members=1, gzip_chunk_bytes=4096)
    keys = (ctypes.c_char_p * len(options))(*[o.encode() for o in options])
    values = np.array(list(options.values()), dtype=np.int64)
    rl = np.ascontiguousarray(w.ds.read_len, dtype=np.uint32)
    bad_path, good_path = w.write("before", cases["crcs of two members exchanged"]), w.write("after", good)
    h = L.hp_text_device_after(bad_path.encode(), good_path.encode(), "\n".join(w.names).encode(), rl.ctypes.data, len(rl), 1, 3, 0,
                               ctypes.cast(keys, ctypes.c_void_p), values.ctypes.data, len(options))
    try:
        info, before = np.zeros(6, dtype=np.int64), np.zeros(2, dtype=np.int64)
        L.hp_paf_device_info(h, info.ctypes.data)
        L.hp_paf_device_before(h, before.ctypes.data)
        assert info[0] == 0 and before[0] & 8, (info, before)
        n = len(w.want["a_id"])
        assert info[1] == 0 and info[2] == -1 and info[3] == n, info
        cols = {f: np.zeros(n, dtype=np.uint32) for f in gg.FIELDS}
        cols["strand"] = np.zeros(n, dtype=np.uint8)
        L.hp_paf_device_copy(h, *[cols[f].ctypes.data for f in gg.FIELDS], cols["strand"].ctypes.data)
        gg.same(cols, w.want)
    finally:
        L.hp_paf_device_free(h)
