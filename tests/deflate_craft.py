"""A deflate encoder that writes what it is told (RFC 1951), for the tests of the device inflaters: streams that zlib's
inflate accepts but its compressor never writes, and streams that differ from a valid one in exactly one thing it refuses.

Parts: a bit writer, a greedy tokeniser whose tokens can be forced, a chooser of code lengths of a requested shape, writers
for dynamic / fixed / stored blocks and raw bits, gzip and BGZF wrappers, and CASES - the table both test files use.  Every
encoder returns (deflate bytes, coverage report); an invalid case also returns the text a decoder that took it would give.
What a test compares the kernels with is never a case's intention but zlib's answer (verdict()) and the host reader's."""
import heapq
import re
import struct
import zlib
from bisect import bisect_right
from collections import Counter

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
OVERLAP_DISTS = (1, 2, 3, 63, 64, 65)


def _bits():
    """a list of bits and its two writers (the handmade block of test_gpu_gzip.py)"""
    out = []

    def put(v, n):                      # n bits of v, least significant first (extra bits, headers)
        for k in range(n):
            out.append((v >> k) & 1)

    def huff(code, n):                  # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            out.append((code >> k) & 1)

    return out, put, huff


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


# ---- tokens -----------------------------------------------------------------------------------------------------------
def is_match(data, p, length, dist):
    if dist < 1 or p - dist < 0 or p + length > len(data):
        return False
    src = data[p - dist:p]
    return data[p:p + length] == (src * (length // dist + 1))[:length]


def tokenise(data, forced=None, boundaries=(), max_len=258, min_dist=1, max_dist=32768, matches=True):
    """data -> tokens: an int is a literal, (length, distance) a match.  Greedy, the latest earlier place of the next three
    bytes.  forced: {text position: (length, distance)} - emitted as given (they must be matches of the data); no token
    crosses a forced position or one of `boundaries`."""
    forced = forced or {}
    n = len(data)
    stops = sorted(set(forced) | set(boundaries) | {n})
    si, i, toks, table = 0, 0, [], {}
    while i < n:
        f = forced.get(i)
        if f is not None:
            assert is_match(data, i, *f), (i, f)
            toks.append(f)
            i += f[0]
            continue
        while stops[si] <= i:
            si += 1
        room = min(stops[si] - i, max_len)
        if matches and room >= 3:
            key = data[i:i + 3]
            j = table.get(key)
            table[key] = i
            if j is not None and min_dist <= i - j <= max_dist:
                length = 3
                while length < room and data[j + length] == data[i + length]:
                    length += 1
                toks.append((length, i - j))
                i += length
                continue
        toks.append(data[i])
        i += 1
    return toks


def text_of(tokens, before=b""):
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out[len(before):])


def token_bytes(t):
    return t[0] if isinstance(t, tuple) else 1


def split(tokens, every, starts=(), pos=0):
    """blocks of at most `every` tokens; a block also begins at every text position in `starts` that is a token boundary"""
    starts = set(starts)
    blocks, cur = [], []
    for t in tokens:
        if cur and (len(cur) >= every or pos in starts):
            blocks.append(cur)
            cur = []
        cur.append(t)
        pos += token_bytes(t)
    blocks.append(cur)
    return blocks


def len_symbol(length, alt258=False):
    if length == 258:
        return (27, 31) if alt258 else (28, 0)
    k = bisect_right(LEN_BASE, length) - 1
    return k, length - LEN_BASE[k]


def dist_symbol(dist):
    k = bisect_right(DIST_BASE, dist) - 1
    return k, dist - DIST_BASE[k]


def frequencies(tokens, alt258=None):
    ll, d = Counter({256: 1}), Counter()
    for i, t in enumerate(tokens):
        if isinstance(t, tuple):
            ll[257 + len_symbol(t[0], bool(alt258) and i % 2 == 1)[0]] += 1
            d[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    return ll, d


# ---- code lengths -------------------------------------------------------------------------------------------------------
def kraft(lens):
    """the sum of 2^-length over the codes, in units of 2^-15"""
    return sum(1 << (15 - l) for l in lens if l)


def optimal(freq, n, limit=15):
    """length-limited Huffman over the symbols of freq; a lone symbol gets a neighbour so that the set is complete"""
    freq = {s: f for s, f in freq.items() if f > 0}
    if len(freq) < 2:
        for s in range(n):
            if len(freq) >= 2:
                break
            freq.setdefault(s, 0)
    heap = [(f, s, (s,)) for s, f in sorted(freq.items())]
    heapq.heapify(heap)
    depth = dict.fromkeys(freq, 0)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    for s in depth:
        depth[s] = min(depth[s], limit)
    full = 1 << limit
    total = sum(1 << (limit - l) for l in depth.values())
    order = sorted(depth, key=lambda s: (freq[s], s))
    while total > full:                                     # too many short codes: lengthen the rarest that can be
        s = next(s for s in order if depth[s] < limit)
        total -= 1 << (limit - depth[s] - 1)
        depth[s] += 1
    while total < full:                                     # room left: shorten the most frequent that fits
        s = next(s for s in reversed(order) if (1 << (limit - depth[s])) <= full - total)
        total += 1 << (limit - depth[s])
        depth[s] -= 1
    lens = [0] * n
    for s, l in depth.items():
        lens[s] = l
    return lens


def _spread(freq, n, depths, pad_from):
    """depths (leaves of a complete tree) over the symbols: the longest to the most frequent, what is left to unused symbols"""
    used = sorted((s for s in freq if freq[s] > 0), key=lambda s: (-freq[s], s))
    spare = [s for s in range(pad_from, n) if freq.get(s, 0) == 0] + [s for s in range(pad_from) if freq.get(s, 0) == 0]
    assert len(depths) >= len(used) and len(depths) - len(used) <= len(spare), (len(depths), len(used))
    lens = [0] * n
    for s, l in zip(used + spare, sorted(depths, reverse=True)):
        lens[s] = l
    return lens


def comb(freq, n, pad_from=0):
    """1, 2, 3 .. 14, 15, 15 over at most 16 used symbols (unused ones take the short end)"""
    return _spread(freq, n, list(range(1, 16)) + [15], pad_from)


def deep(freq, n, seed, limit=15, need=(), pad_from=0, leaves=None):
    """random leaf splitting down to `limit`, deep leaves split first; every length in `need` occurs among the used symbols"""
    used = sum(1 for f in freq.values() if f > 0)
    need = sorted(need)[len(need) - min(len(need), max(0, used - 1)):]      # (as many of them as there are symbols to carry them)
    leaves = max(used, leaves or 0, limit + 1)
    assert leaves <= n
    for attempt in range(1000):
        rng = np.random.default_rng(seed * 1000 + attempt)
        d = [0]
        while len(d) < leaves:
            open_ = [k for k, x in enumerate(d) if x < limit]
            w = np.array([3.0 ** d[k] for k in open_])
            k = open_[int(rng.choice(len(open_), p=w / w.sum()))]
            d[k] += 1
            d.append(d[k])
        if set(need) <= set(sorted(d, reverse=True)[:used]):
            return _spread(freq, n, d, pad_from)
    raise AssertionError("no tree with lengths %r" % (need,))


def codes_of(lens):
    """canonical codes of the lengths, bit-reversed for the writer: {symbol: (bits, length)}.  Sets that are not complete
    get the codes the counting rule gives (an over-subscribed set's wrap round)."""
    count = Counter(l for l in lens if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (_rev(nxt[l] & ((1 << l) - 1), l), l)
            nxt[l] += 1
    return out


def run_lengths(seq, style, nlen=None):
    """the code-length sequence as code-length symbols [(symbol, extra value)]: style none (no repeat code), zlib (the
    longest repeat first), extremes (repeat counts at both ends of their ranges: 18 as 138 / 11, 17 as 10 / 3, 16 as 6 / 3;
    a run that crosses `nlen` gets a 16 across it)"""
    if style == "none":
        return [(v, None) for v in seq]
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if style == "extremes" and nlen is not None and i <= nlen - 2 and j >= nlen + 2 and v == 0:
            out += run_lengths(seq[i:nlen - 2], style) + [(v, None), (16, 0)]      # lengths nlen-1, nlen, nlen+1 by one 16
            i = nlen + 2
            continue
        if v == 0:
            sizes = (138, 11, 10, 3) if style == "extremes" else tuple(range(138, 2, -1))
        else:
            out.append((v, None))
            run -= 1
            i += 1
            sizes = (6, 3) if style == "extremes" else (6, 5, 4, 3)
        while run >= 3:
            c = next(c for c in sizes if c <= run and (style != "extremes" or run - c == 0 or run - c >= 3 or c == sizes[-1]))
            out.append((18, c - 11) if v == 0 and c >= 11 else (17, c - 3) if v == 0 else (16, c - 3))
            run -= c
            i += c
        out += [(v, None)] * run
        i += run
    return out


# ---- the writer -------------------------------------------------------------------------------------------------------
def new_report():
    return {"ll": Counter(), "dist": Counter(), "cl": Counter(), "len_syms": set(), "dist_syms": set(), "repeats": Counter(),
            "cross16": 0, "blocks": 0, "matches": 0, "ends": Counter(), "hlit": set(), "hdist": set(), "hclen": set(),
            "stored": Counter(), "starts": []}


class Writer:
    """deflate blocks, bit by bit.  report: symbols coded per code length and alphabet (ll, dist, cl), the length and
    distance symbols used, repeat codes as (symbol, count), blocks, the bit alignments at which coded blocks ended, stored
    blocks per size, and starts: (bit offset in the stream, first token) of every dynamic block."""

    def __init__(self):
        self.out, self.acc, self.n, self.report = bytearray(), 0, 0, new_report()

    def put(self, v, n):                        # n bits of v, least significant first; a Huffman code comes bit-reversed
        self.acc |= v << self.n
        self.n += n
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def huff(self, code, n):                    # most significant bit first
        self.put(_rev(code, n), n)

    def raw(self, bits):
        for b in bits:
            self.put(int(b), 1)

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.put(0, -self.bit_length() % 8)

    def getvalue(self):
        self.align()
        return bytes(self.out) + self.acc.to_bytes(self.n // 8, "little")

    def stored(self, data, final=False, length=None, nlen=None):
        assert len(data) <= 65535
        self.report["blocks"] += 1
        self.report["stored"][len(data)] += 1
        self.put(int(final), 1)
        self.put(0, 2)
        self.align()
        length = len(data) if length is None else length
        self.put(length, 16)
        self.put(length ^ 0xFFFF if nlen is None else nlen, 16)
        self.out += self.acc.to_bytes(self.n // 8, "little") + bytes(data)      # (byte aligned here)
        self.acc = self.n = 0

    def symbols(self, tokens, ll, dist, alt258=False, eob=True):
        """the tokens and the end-of-block code through the codes ll / dist ({symbol: (reversed bits, length)})"""
        rep = self.report
        for i, t in enumerate(tokens):
            if isinstance(t, tuple):
                k, extra = len_symbol(t[0], alt258 and i % 2 == 1)
                self.put(*ll[257 + k])
                self.put(extra, LEN_EXTRA[k])
                dk, dextra = dist_symbol(t[1])
                self.put(*dist[dk])
                self.put(dextra, DIST_EXTRA[dk])
                rep["ll"][ll[257 + k][1]] += 1
                rep["dist"][dist[dk][1]] += 1
                rep["len_syms"].add((257 + k, extra) if k == 27 and extra == 31 else 257 + k)
                rep["dist_syms"].add(dk)
                rep["matches"] += 1
            else:
                self.put(*ll[t])
                rep["ll"][ll[t][1]] += 1
        if eob:
            self.put(*ll[256])
            rep["ll"][ll[256][1]] += 1
        rep["ends"][self.bit_length() % 8] += 1

    def fixed(self, tokens, final=False, extra=()):
        """a fixed-codes block; extra: (code, bits) pairs written MSB first behind the tokens (symbols no token can name)"""
        self.report["blocks"] += 1
        self.put(int(final), 1)
        self.put(1, 2)
        self.symbols(tokens, codes_of(FIXED_LL), codes_of([5] * 30), eob=False)
        for code, n in extra:
            self.huff(code, n)
        self.symbols([], codes_of(FIXED_LL), codes_of([5] * 30))

    def header(self, ll_lens, d_lens, hclen=None, cl_lens=None, rle="zlib", items=None, hlit_field=None, hdist_field=None):
        """HLIT, HDIST, HCLEN, the code-length code and the lengths (RFC 1951 3.2.7).  The counts are len(ll_lens) and
        len(d_lens); items: the code-length symbols as given instead of run_lengths'; cl_lens: the code-length code's lengths"""
        rep = self.report
        nlen, ndist = len(ll_lens), len(d_lens)
        if items is None:
            items = run_lengths(list(ll_lens) + list(d_lens), rle, nlen)
        if cl_lens is None:
            cl_lens = optimal(Counter(s for s, _ in items), 19, 7)
        need = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
        hclen = max(4, need) if hclen is None else hclen
        assert 4 <= hclen <= 19 and hclen >= need
        self.put(nlen - 257 if hlit_field is None else hlit_field, 5)
        self.put(ndist - 1 if hdist_field is None else hdist_field, 5)
        self.put(hclen - 4, 4)
        for k in range(hclen):
            self.put(cl_lens[CL_ORDER[k]], 3)
        cl = codes_of(cl_lens)
        at = 0
        for s, extra in items:
            self.put(*cl[s])
            rep["cl"][cl[s][1]] += 1
            if s >= 16:
                bits, base = {16: (2, 3), 17: (3, 3), 18: (7, 11)}[s]
                self.put(extra, bits)
                rep["repeats"][(s, base + extra)] += 1
                rep["cross16"] += s == 16 and at < nlen < at + base + extra
                at += base + extra
            else:
                at += 1
        rep["hlit"].add(nlen)
        rep["hdist"].add(ndist)
        rep["hclen"].add(hclen)

    def dynamic(self, tokens, final=False, ll_lens=None, d_lens=None, hlit=None, hdist=None, alt258=False, eob=True, **header):
        """a dynamic block of the tokens; the lengths default to optimal ones, hlit / hdist pad the counts with zeros"""
        fl, fd = frequencies(tokens, alt258)
        ll_lens = optimal(fl, 286) if ll_lens is None else list(ll_lens)
        d_lens = optimal(fd, 30) if d_lens is None else list(d_lens)
        nlen = max(257, max(s for s in range(len(ll_lens)) if ll_lens[s]) + 1) if hlit is None else hlit
        ndist = max(1, max([s for s in range(len(d_lens)) if d_lens[s]] + [0]) + 1) if hdist is None else hdist
        ll_lens = (ll_lens + [0] * nlen)[:nlen]
        d_lens = (d_lens + [0] * ndist)[:ndist]
        self.report["blocks"] += 1
        self.report["starts"].append((self.bit_length(), tokens[0] if tokens else None))
        self.put(int(final), 1)
        self.put(2, 2)
        self.header(ll_lens, d_lens, **header)
        self.symbols(tokens, codes_of(ll_lens), codes_of(d_lens), alt258, eob)


# ---- wrappers ---------------------------------------------------------------------------------------------------------
def gz_member(body, data, name=None):
    """a gzip member around raw deflate bytes `body` of text `data` (FNAME when a name is given)"""
    h = b"\x1f\x8b\x08" + (b"\x08" if name else b"\x00") + b"\x00" * 4 + b"\x00\xff" + (name + b"\x00" if name else b"")
    return h + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def bgzf_member(body, data):
    """a BGZF member (SAM specification 4.1) around raw deflate bytes; None where it would exceed 64 KB"""
    total = 18 + len(body) + 8
    if total > 65536 or len(data) > 65536:
        return None
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1) + body +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf_file(text, encode, size=60000, cuts=(), eof=True):
    """text as BGZF members of at most `size` bytes of text (a number, or a function of the member's index), each through
    encode(text) -> (deflate bytes, report, ...); a member also begins at every position in `cuts`; a member whose bytes do
    not fit is halved.  -> (file bytes, merged report; its "member_text": the members' text sizes)"""
    out, i, rep = [], 0, new_report()
    rep["member_text"] = []
    cuts = sorted(c for c in cuts if 0 < c < len(text)) + [len(text)]
    while i < len(text):
        n = min(size(len(out)) if callable(size) else size, next(c for c in cuts if c > i) - i)
        while True:
            res = encode(text[i:i + n])
            m = bgzf_member(res[0], text[i:i + n])
            if m is not None:
                break
            n = (n + 1) // 2
        out.append(m)
        merge(rep, res[1])
        rep["member_text"].append(n)
        i += n
    if eof:
        out.append(bgzf_member(b"\x03\x00", b""))
    return b"".join(out), rep


def merge(into, rep):
    for k, v in rep.items():
        if k not in into:
            continue
        if isinstance(v, Counter):
            into[k].update(v)
        elif isinstance(v, set):
            into[k] |= v
        elif isinstance(v, list):                   # (offsets within one stream: not kept across members)
            continue
        else:
            into[k] += v
    return into


def verdict(body):
    """zlib's inflate on raw deflate bytes: the text, or None where it refuses them or they end unfinished"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(body)
    except zlib.error:
        return None
    return text if d.eof else None


# ---- texts ------------------------------------------------------------------------------------------------------------
FAR_LITERALS = 32800


def far_copies():
    """(length, distance) pairs that use every distance symbol and every length symbol, extra bits drawn at random, the
    longest distance and both ends of a few ranges among them"""
    rng = np.random.default_rng(99)
    out = []
    for k in range(30):
        dist = DIST_BASE[k] + int(rng.integers(0, 1 << DIST_EXTRA[k]))
        j = k % 29
        out.append((LEN_BASE[j] + int(rng.integers(0, 1 << LEN_EXTRA[j])), dist))
    return out + [(258, 32768), (257, 24577), (227, 24576), (3, 32768)]


def overlap_tag(d):
    return b"\tOV:Z:" + (bytes(40 + k for k in range(d)) * (270 // d + 2))[:d + 258 + 3 + 4]


def far_tag():
    rng = np.random.default_rng(7)
    out = bytearray(rng.integers(40, 111, FAR_LITERALS).astype(np.uint8).tobytes())
    for length, dist in far_copies():
        for _ in range(length):
            out.append(out[-dist])
    return b"\tFC:Z:" + bytes(out)


def tagged(text, stride=400):
    """PAF text with tags behind some lines' columns: OV:Z: runs of period 1, 2, 3, 63, 64, 65 (a match at that distance
    overlaps itself) every `stride` lines, and one FC:Z: tag of 32 800 random bytes followed by copies of them at every
    distance symbol's distances.  -> (text, where the FC line begins)"""
    lines = text.splitlines(keepends=True)
    far_line, at, out = len(lines) // 2, 0, []
    for i, line in enumerate(lines):
        if i == far_line:
            far_at = at
            line = line[:-1] + far_tag() + b"\n"
        elif i % stride == stride // 2:
            line = line[:-1] + overlap_tag(OVERLAP_DISTS[(i // stride) % 6]) + b"\n"
        out.append(line)
        at += len(line)
    return b"".join(out), far_at


def overlap_forces(data, short=True):
    """{position: (258, d) and then (3, d)} inside every OV:Z: run of the data whose period d is one of OVERLAP_DISTS"""
    forced = {}
    for m in re.finditer(rb"OV:Z:([^\n]*)", data):
        c, s = m.group(1), m.start(1)
        for d in OVERLAP_DISTS:
            if len(c) >= d + 261 and c[d:] == c[:-d]:
                forced[s + d] = (258, d)
                if short:
                    forced[s + d + 258] = (3, d)
                break
    return forced


def far_forces(data):
    """the copies behind the FC:Z: tag's literals as forced matches, those the data holds whole"""
    forced = {}
    m = re.search(rb"FC:Z:([^\n]*)", data)
    if m and len(m.group(1)) > FAR_LITERALS:
        p = m.start(1) + FAR_LITERALS
        for length, dist in far_copies():
            if is_match(data, p, length, dist) and p + length <= m.end(1):
                forced[p] = (length, dist)
            p += length
    return forced


# ---- the cases --------------------------------------------------------------------------------------------------------
_TOKENS = {}


def tokens_of(text, **kw):
    """tokenise, remembered per text and options (the cases share few tokenisations)"""
    key = (hash(text), len(text), repr(sorted(kw.items())))
    if key not in _TOKENS:
        if len(_TOKENS) > 64:
            _TOKENS.clear()
        _TOKENS[key] = tokenise(text, **kw)
    return _TOKENS[key]


def blocks_of(text, every=4000, **kw):
    return split(tokens_of(text, **kw), every)


def _each(text, blocks, write):
    """write(w, tokens, final, k) per block -> (bytes, report)"""
    w = Writer()
    for k, b in enumerate(blocks):
        write(w, b, k == len(blocks) - 1, k)
    return w.getvalue(), w.report


def long_lit_codes(text):
    def write(w, b, final, k):
        fl, _ = frequencies(b)
        w.dynamic(b, final, ll_lens=deep(fl, 286, 11 + k, need=(11, 12, 13, 14, 15), pad_from=128))
    return _each(text, blocks_of(text), write)


def long_dist_codes(text):
    def write(w, b, final, k):
        _, fd = frequencies(b)
        w.dynamic(b, final, d_lens=deep(fd, 30, 5 + k, need=(9, 10, 11, 12, 13, 14, 15), leaves=24) if len(fd) >= 8 else None)
    return _each(text, blocks_of(text), write)


def boundary_codes(text):
    def write(w, b, final, k):
        fl, fd = frequencies(b)
        w.dynamic(b, final, ll_lens=deep(fl, 286, 3 + k, limit=11, need=(10, 11), pad_from=128),
                  d_lens=deep(fd, 30, 3 + k, limit=9, need=(8, 9)) if len(fd) >= 8 else None)
    return _each(text, blocks_of(text), write)


def comb_case(text):
    """literals only; a block ends where a 17th symbol (the end-of-block code included) would come in"""
    blocks, cur, seen = [], [], set()
    for t in tokens_of(text, matches=False):
        if t not in seen and len(seen) == 15 or len(cur) >= 4000:
            blocks.append(cur)
            cur, seen = [], set()
        seen.add(t)
        cur.append(t)
    blocks.append(cur)

    def write(w, b, final, k):
        fl, _ = frequencies(b)
        w.dynamic(b, final, ll_lens=comb(fl, 286, pad_from=128), d_lens=[0])
    return _each(text, blocks, write)


def one_distance_code(text):
    """every match at a distance of one symbol (4097 - 6144, 11 extra bits; where a block has none: distance 1 of the
    OV:Z: runs), the symbol's code the lone one-bit code of the block"""
    toks = tokens_of(text, min_dist=4097, max_dist=6144)

    def write(w, b, final, k):
        d = [0] * 30
        d[24] = 1
        w.dynamic(b, final, d_lens=d, hdist=25 if k % 2 else 30)
    return _each(text, split(toks, 4000), write)


def no_distance_code(text):
    return _each(text, split(tokens_of(text, matches=False), 4000), lambda w, b, final, k: w.dynamic(b, final, d_lens=[0], hdist=1))


def max_header(text):
    def write(w, b, final, k):
        fl, fd = frequencies(b)
        ll, d = optimal(fl, 286), optimal(fd, 30)
        items = run_lengths(ll + d, "zlib" if k % 2 else "none")
        w.dynamic(b, final, ll_lens=ll, d_lens=d, hlit=286, hdist=30, hclen=19, items=items,
                  cl_lens=deep(Counter(s for s, _ in items), 19, 2 + k, limit=7, need=(7,), leaves=10))
    return _each(text, blocks_of(text), write)


def min_header(text):
    """HCLEN 5, the least a valid block can have (HCLEN 4 leaves only the symbols 16, 17, 18 and 0, lengths that are all zero:
    no end-of-block code, and zlib refuses that - hclen_4 among the invalid cases): 256 codes of 8 bits, literals only"""
    ll = [8] * 255 + [0, 8]

    def write(w, b, final, k):
        w.dynamic(b, final, ll_lens=ll, d_lens=[0], hdist=1, hclen=5, rle="zlib" if k % 2 else "none",
                  cl_lens=None if k % 2 else [1 if s in (0, 8) else 0 for s in range(19)])
    return _each(text, split(tokens_of(text, matches=False), 4000), write)


def repeat_codes(text):
    """lengths shaped so that every extreme repeat occurs: the 16 unused literals 11 - 26 take a length of their own (a run of
    16 equal lengths: 16 x 6, 6, 3), the zeros of symbols 115 - 255 give 18 x 138 and 17 x 3, other runs 18 x 11 and 17 x 10;
    no match of length 195 or more or distance below 4, so zeros lie on both sides of HLIT 286 and one 16 crosses it"""
    def write(w, b, final, k):
        fl, fd = frequencies(b)
        ll = [l + 1 if l else 0 for l in optimal(fl, 286, 14)]
        for s in range(11, 27):
            ll[s] = 5
        w.dynamic(b, final, ll_lens=ll, d_lens=optimal(fd, 30), hlit=286, hdist=30, rle="extremes")
    return _each(text, blocks_of(text, max_len=194, min_dist=4), write)


def len258_two_ways(text):
    toks = tokens_of(text, forced=overlap_forces(text, short=False))
    return _each(text, split(toks, 4000), lambda w, b, final, k: w.dynamic(b, final, alt258=True))


def all_length_and_distance_symbols(text):
    return _each(text, split(tokens_of(text, forced=far_forces(text)), 4000), lambda w, b, final, k: w.dynamic(b, final))


def overlapping_copies(text):
    return _each(text, split(tokens_of(text, forced=overlap_forces(text)), 4000), lambda w, b, final, k: w.dynamic(b, final))


def stored_mix(text, sizes=(0, 1, 4095, 4096, 4097)):
    """eight rounds of a dynamic block of about 2000 bytes (tokenised on its own, shortened byte by byte until it ends at bit
    alignment 0, 1 .. 7 in turn) and a stored block of the next size; the rest of the text in large dynamic blocks"""
    w, pos = Writer(), 0
    for k in range(8):
        size = sizes[k % len(sizes)]
        if pos + 2100 + size >= len(text):                  # (a text too short for all eight: a BGZF member)
            break
        for n in range(2100, 2000, -1):
            toks, t = tokenise(text[pos:pos + n]), Writer()
            t.dynamic(toks)
            if (w.bit_length() + t.bit_length()) % 8 == k:
                break
        else:
            raise AssertionError("no block ends at alignment %d" % k)
        w.dynamic(toks)
        w.stored(text[pos + n:pos + n + size])
        pos += n + size
    rest = split(tokenise(text[pos:]), 4000)
    for i, b in enumerate(rest):
        w.dynamic(b, i == len(rest) - 1)
    return w.getvalue(), w.report


def stored_mix_65535(text):
    return stored_mix(text, sizes=(0, 1, 4095, 4096, 4097, 65535))


def empty_blocks(text):
    """runs of empty dynamic, fixed and stored blocks in front of, between and behind the text's blocks; the final block an
    empty stored one"""
    w = Writer()

    def run(n):
        for k in range(n):
            (lambda: w.dynamic([]), lambda: w.fixed([]), lambda: w.stored(b""))[k % 3]()
    run(7)
    for k, b in enumerate(blocks_of(text)):
        w.dynamic(b)
        run(k % 5)
    run(9)
    w.stored(b"", final=True)
    return w.getvalue(), w.report


def tiny_blocks(text):
    return _each(text, blocks_of(text, every=10), lambda w, b, final, k: w.dynamic(b, final))


MARKER_WIDTH = 1024                         # bytes per line of marker_text: 32 lines are deflate's window
MARKER_KINDS = ((258, 1), (258, 32768), (3, 2))


def marker_text(text, n_lines):
    """the first n_lines lines of PAF text, each padded by an MC:Z: tag to 1024 bytes that end in: 258 random bytes that are
    the same in every 32nd line (a copy at distance 32 768), 40 bytes of the line's own, 259 x (a run at distance 1), 40
    bytes of the line's own, ababa (aba: length 3 at distance 2)"""
    rng = np.random.default_rng(5)
    shared = [rng.integers(40, 111, 258).astype(np.uint8).tobytes() for _ in range(32768 // MARKER_WIDTH)]
    out = []
    for i, line in enumerate(text.splitlines(keepends=True)[:n_lines]):
        own = rng.integers(40, 111, 80).astype(np.uint8).tobytes()
        tail = shared[i % len(shared)] + own[:40] + b"x" * 259 + own[40:] + b"ababa\n"
        head = line[:-1] + b"\tMC:Z:"
        assert len(head) + len(tail) < MARKER_WIDTH
        out.append(head + b"." * (MARKER_WIDTH - len(head) - len(tail)) + tail)
    return b"".join(out)


def marker_forces(data):
    """the three copies in every line of marker_text, where the data holds them"""
    forced = {}
    for end in range(MARKER_WIDTH, len(data) + 1, MARKER_WIDTH):
        if data[end - 6:end] != b"ababa\n":
            return {}
        for p, f in ((end - 6 - 40 - 259 - 40 - 258, (258, 32768)), (end - 6 - 40 - 258, (258, 1)), (end - 4, (3, 2))):
            if is_match(data, p, *f):
                forced[p] = f
    return forced


def marker_copies(text):
    """gzip only: dynamic blocks that begin with a match reaching in front of the block: at every forced copy - distance 1
    at length 258, distance 32 768, distance length - 1 in the lines of marker_text, the OV:Z: and FC:Z: copies of tagged() -
    and otherwise every 4000 tokens"""
    forced = marker_forces(text)
    forced.update(overlap_forces(text))
    forced.update(far_forces(text))
    toks = tokens_of(text, forced=forced)
    return _each(text, split(toks, 4000, starts=forced), lambda w, b, final, k: w.dynamic(b, final))


def chunk_first_blocks(starts, chunk):
    """what the first dynamic block that begins in each chunk of `chunk` deflate bytes (but the first chunk) opens with: a
    Counter of first tokens - the block starts the gzip inflater's find pass takes for its chunks (chunks are counted from
    the deflate bytes' start, as starts' bit offsets are)"""
    first = {}
    for bit, token in starts:
        c = bit // (8 * chunk)
        if c >= 1 and c not in first:
            first[c] = token
    return Counter(first.values())


def plain(text):
    """nothing special: optimal codes, zlib's choice of repeat codes"""
    return _each(text, blocks_of(text), lambda w, b, final, k: w.dynamic(b, final))


def bgzf_with_bad_member(text, name, place, size=60000):
    """text as BGZF members, the second one changed as invalid(name, ., place) does and its trailer that of the text a
    tolerant decoder would give"""
    body, _, got = invalid(name, text[size:2 * size], place)
    assert verdict(body) is None
    bad = bgzf_member(body, got or text[size:2 * size])      # (a member of no text is an end-of-file marker, not a broken member)
    assert bad is not None and len(text) > 2 * size
    return bgzf_file(text[:size], plain, size, eof=False)[0] + bad + bgzf_file(text[2 * size:], plain, size)[0]


def paf_text(ds, path, n_lines):
    """the first n_lines lines of the data set's PAF, tagged() -> (text, where its FC:Z: line begins)"""
    ds.write_paf(path)
    with open(path, "rb") as f:
        return tagged(b"".join(f.read().splitlines(keepends=True)[:n_lines]))


def _share(counter, lo):
    return sum(n for l, n in counter.items() if l >= lo) / max(1, sum(counter.values()))


def covers(name, rep):
    """asserts the conditions that keep case `name` from passing without the branch it is there for, on an encode's report
    (a BGZF file's merged report: the conditions hold over its members together)"""
    if name == "long_lit_codes":
        assert _share(rep["ll"], 11) >= 0.5 and all(rep["ll"][l] > 0 for l in range(11, 16)), rep["ll"]
    if name == "long_dist_codes":
        assert _share(rep["dist"], 9) >= 0.5 and all(rep["dist"][l] > 0 for l in range(9, 16)), rep["dist"]
    if name == "boundary_codes":
        assert min(rep["ll"][10], rep["ll"][11], rep["dist"][8], rep["dist"][9]) >= 10, (rep["ll"], rep["dist"])
    if name == "comb":
        assert all(rep["ll"][l] > 0 for l in range(1, 16)) and _share(rep["ll"], 11) >= 0.5, rep["ll"]
    if name == "one_distance_code":
        assert rep["matches"] >= 10 and set(rep["dist"]) == {1} and rep["dist_syms"] == {24}
    if name == "no_distance_code":
        assert rep["matches"] == 0 and rep["hdist"] == {1}
    if name == "max_header":
        assert rep["hlit"] == {286} and rep["hdist"] == {30} and rep["hclen"] == {19} and rep["cl"][7] > 0
    if name == "min_header":
        assert rep["hclen"] == {5} and rep["hlit"] == {257}
    if name == "repeat_codes":
        for key in ((16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)):
            assert rep["repeats"][key] > 0, (key, rep["repeats"])
        assert rep["cross16"] > 0
    if name == "len258_two_ways":
        assert {285, (284, 31)} <= rep["len_syms"]
    if name == "all_length_and_distance_symbols":
        assert len(rep["len_syms"]) == 29 and len(rep["dist_syms"]) == 30
    if name == "overlapping_copies":
        assert rep["matches"] > 0
    if name in ("stored_mix", "stored_mix_65535"):
        sizes = (0, 1, 4095, 4096, 4097) + ((65535,) if name == "stored_mix_65535" else ())
        assert set(rep["ends"]) == set(range(8)) and all(rep["stored"][n] >= 1 for n in sizes), (rep["ends"], rep["stored"])
    if name == "empty_blocks":
        assert rep["stored"][0] >= 5
    if name == "tiny_blocks":
        assert rep["blocks"] * 10 >= sum(rep["ll"].values()) - rep["blocks"]
    if name == "marker_copies":
        for chunk in (1024, 4096):              # several of the chunks' first blocks open with each kind of copy
            first = chunk_first_blocks(rep["starts"], chunk)
            assert all(first[kind] >= 3 for kind in MARKER_KINDS), (chunk, first)


VALID = {f.__name__: f for f in (long_lit_codes, long_dist_codes, boundary_codes, one_distance_code, no_distance_code, max_header,
                                 min_header, repeat_codes, len258_two_ways, all_length_and_distance_symbols, overlapping_copies,
                                 stored_mix, empty_blocks, tiny_blocks)}
VALID["comb"] = comb_case
GZIP_ONLY = {"stored_mix_65535": stored_mix_65535, "marker_copies": marker_copies}


# ---- invalid cases: one change in one block of an otherwise valid stream ---------------------------------------------
def _plan(b):
    fl, fd = frequencies(b)
    return optimal(fl, 286), optimal(fd, 30)


def _bump(lens, by, freq):
    """the rarest used symbol's length changed by `by`: -1 over-subscribes a complete set, +1 leaves it incomplete"""
    lens = list(lens)
    s = min((s for s in range(len(lens)) if lens[s] > 1 and lens[s] + by <= 15), key=lambda s: (freq.get(s, 0), -lens[s], s))
    lens[s] += by
    return lens


def _bad_ll(by):
    def bad(w, b, final):
        ll, d = _plan(b)
        w.dynamic(b, final, ll_lens=_bump(ll, by, frequencies(b)[0]), d_lens=d)
    return bad


def _bad_dist(by):
    def bad(w, b, final):
        ll, d = _plan(b)
        w.dynamic(b, final, ll_lens=ll, d_lens=_bump(d, by, frequencies(b)[1]))
    return bad


def _bad_cl(by):
    def bad(w, b, final):
        ll, d = _plan(b)
        items = run_lengths(ll[:max(s for s in range(286) if ll[s]) + 1] + d, "zlib")
        cl = optimal(Counter(s for s, _ in items), 19, 7)
        w.dynamic(b, final, ll_lens=ll, d_lens=d, hdist=30, cl_lens=_bump(cl, by, Counter(s for s, _ in items)))
    return bad


def _incomplete_dist_two_bits(w, b, final):
    d = [0] * 30
    d[24] = 2                                   # the lone distance code two bits long
    w.dynamic(b, final, d_lens=d)


def _no_end_of_block_code(w, b, final):
    """the end-of-block code's place in a complete set given to the unused literal 255; the block ends without it"""
    fl, _ = frequencies(b)
    fl[255] = fl.pop(256)
    ll = optimal(fl, 286)
    w.dynamic(b, final, ll_lens=ll, eob=False)


def _repeat16_first(w, b, final):
    ll, d = _plan(b)
    seq = ll[:max(s for s in range(286) if ll[s]) + 1] + d
    assert seq[:4] == [0, 0, 0, 0]              # (a decoder that takes "the length before the first" as 0 reads the same lengths)
    items = [(16, 0)] + run_lengths(seq[3:], "zlib")
    w.dynamic(b, final, ll_lens=ll, d_lens=d, hdist=30, items=items, cl_lens=optimal(Counter(s for s, _ in items), 19, 7))


def _repeat_overflow(w, b, final):
    """the zeros that end the distance lengths, written by a repeat of one more than there are"""
    ll, d = _plan(b)
    d = d[:max(s for s in range(30) if d[s]) + 1] + [0] * 4
    d = d[:30]
    tail = 0
    while d[-1 - tail] == 0:
        tail += 1
    assert tail >= 3
    nl = max(s for s in range(286) if ll[s]) + 1
    items = run_lengths(ll[:nl] + d[:len(d) - tail], "zlib") + [(17, tail + 1 - 3)]
    w.dynamic(b, final, ll_lens=ll, d_lens=d, hdist=len(d), items=items, cl_lens=optimal(Counter(s for s, _ in items), 19, 7))


def _hlit_287(w, b, final):
    ll, d = _plan(b)
    w.dynamic(b, final, ll_lens=ll + [0], d_lens=d, hlit=287)       # 287 lengths follow, as the field says


def _hdist_31(w, b, final):
    ll, d = _plan(b)
    w.dynamic(b, final, ll_lens=ll, d_lens=d + [0], hdist=31)


def _hclen_4(w, b, final):
    """HCLEN 4: only zero lengths can be written, so there is no end-of-block code and zlib refuses the block"""
    w.put(int(final), 1)
    w.put(2, 2)
    w.header([0] * 257, [0], hclen=4, cl_lens=[1 if s in (0, 18) else 0 for s in range(19)])


def _btype3(w, b, final):
    w.put(int(final), 1)
    w.put(3, 2)
    ll, d = _plan(b)
    w.header(ll[:max(s for s in range(286) if ll[s]) + 1], d)
    w.symbols(b, codes_of(ll), codes_of(d))


def _fixed_len_286(w, b, final):
    w.fixed(b[:200], extra=[(0xC0 + 6, 8), (0, 5)])                 # symbol 286 (8 bits, 11000110) and a distance code behind it
    w.dynamic(b[200:], final)


def _fixed_dist_30(w, b, final):
    w.fixed(b[:200], extra=[(1, 7), (30, 5)])                       # length 3, distance symbol 30
    w.dynamic(b[200:], final)


def _absent_code(w, b, final):
    """a lone one-bit distance code (0); from the block's first match on the matches are written with the bit 1"""
    d = [0] * 30
    d[24] = 1
    ll = optimal(frequencies(b)[0], 286)
    w.report["blocks"] += 1
    w.put(int(final), 1)
    w.put(2, 2)
    nl = max(s for s in range(286) if ll[s]) + 1
    w.header(ll[:nl], d)
    codes = codes_of(d)
    k = next(i for i, t in enumerate(b) if isinstance(t, tuple))
    w.symbols(b[:k], codes_of(ll), codes, eob=False)
    w.symbols(b[k:], codes_of(ll), {24: (1, 1)})


def _cut_header(w, b, final):
    """the block's header and nothing behind it: the stream ends inside the code lengths"""
    ll, d = _plan(b)
    w.put(int(final), 1)
    w.put(2, 2)
    w.header(ll[:max(s for s in range(286) if ll[s]) + 1], d, rle="none")       # (invalid() drops the stream's last 12 bytes)


_ONE_DISTANCE = dict(min_dist=4097, max_dist=6144)
INVALID = {
    "oversubscribed_ll": (_bad_ll(-1), {}), "oversubscribed_dist": (_bad_dist(-1), {}), "oversubscribed_cl": (_bad_cl(-1), {}),
    "incomplete_ll": (_bad_ll(+1), {}), "incomplete_dist_two_bits": (_incomplete_dist_two_bits, _ONE_DISTANCE),
    "incomplete_cl": (_bad_cl(+1), {}), "no_end_of_block_code": (_no_end_of_block_code, {}),
    "repeat16_first": (_repeat16_first, {}), "repeat_overflow": (_repeat_overflow, dict(max_dist=4096)),
    "hlit_287": (_hlit_287, {}), "hdist_31": (_hdist_31, {}), "hclen_4": (_hclen_4, {}), "btype3": (_btype3, {}),
    "fixed_len_286": (_fixed_len_286, {}), "fixed_dist_30": (_fixed_dist_30, {}),
    "absent_code_of_one_code_set": (_absent_code, _ONE_DISTANCE), "header_cut_by_end_of_input": (_cut_header, {}),
}
SPECIAL_INVALID = ("stored_nlen", "stored_past_end", "distance_before_text")
PLACES = ("first", "last")


def invalid(name, text, place):
    """-> (deflate bytes, report, the text a decoder that took the change would give): the change of case `name` in the
    first or the last block of the stream, valid dynamic blocks around it.  A block that cannot end (no end-of-block code, a
    cut header) is the last block either way: in the "first" place the stream is that block alone."""
    assert place in PLACES
    w = Writer()
    if name in ("stored_nlen", "stored_past_end"):
        blocks = blocks_of(text, every=1000)
        k = 0 if place == "first" else len(blocks) - 2
        pos = sum(token_bytes(t) for b in blocks[:k] for t in b)
        for b in blocks[:k]:
            w.dynamic(b)
        if name == "stored_nlen":
            w.stored(text[pos:pos + 500], nlen=(500 ^ 0xFFFF) ^ 0x0100)
            rest = split(tokenise(text[pos + 500:]), 1000)
            for i, b in enumerate(rest):
                w.dynamic(b, i == len(rest) - 1)
            return w.getvalue(), w.report, text
        w.stored(text[pos:pos + 500], final=True, length=600)      # 100 bytes more than the stream holds
        return w.getvalue(), w.report, text[:pos + 500]
    if name == "distance_before_text":
        # first: the stream's first token is a match; last: (gzip: a wave other than the first meets it) the block that
        # begins at text position 20 000 or so opens with a match of distance 30 000
        toks = tokens_of(text)
        at, pos = 0, 0
        if place == "last":
            while pos < 20000:
                pos += token_bytes(toks[at])
                at += 1
        for b in split(toks[:at], 60):
            if b:
                w.dynamic(b)
        w.dynamic([(7, 30000)] + toks[at:at + 60])
        rest = split(toks[at + 60:], 60)
        for i, b in enumerate(rest):
            w.dynamic(b, i == len(rest) - 1)
        n60 = sum(map(token_bytes, toks[:at]))
        return w.getvalue(), w.report, text[:n60] + b"\0" * 7 + text[n60:]
    bad, kw = INVALID[name]
    blocks = blocks_of(text, every=1000, **kw)
    if len(blocks) > 1 and len(blocks[-1]) < 500:
        blocks = blocks[:-2] + [blocks[-2] + blocks[-1]]
    endless = name in ("no_end_of_block_code", "header_cut_by_end_of_input")
    k = 0 if place == "first" else len(blocks) - 1
    if name == "absent_code_of_one_code_set":                           # (the first / last block that holds a match)
        k = [i for i, b in enumerate(blocks) if any(isinstance(t, tuple) for t in b)][0 if place == "first" else -1]
    if endless and place == "first":
        blocks = blocks[:1]
    for i, b in enumerate(blocks):
        final = i == len(blocks) - 1
        if i == k:
            bad(w, b, final)
        elif name in ("absent_code_of_one_code_set", "incomplete_dist_two_bits"):
            d = [0] * 30
            d[24] = 1
            w.dynamic(b, final, d_lens=d)
        else:
            w.dynamic(b, final)
    body, got = w.getvalue(), text
    if name == "header_cut_by_end_of_input":
        body, got = body[:-12], text_of([t for b in blocks[:-1] for t in b])
    elif endless and place == "first":
        got = text_of(blocks[0])
    return body, w.report, got


INVALID_NAMES = tuple(INVALID) + SPECIAL_INVALID
