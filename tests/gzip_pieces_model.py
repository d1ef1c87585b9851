"""A model of what the ranks of a sharded run hand each other when they take one gzip member together (option gzip_in_pieces):
a deflate decoder that remembers where every byte of the text came from, the pieces' out-windows in marker form derived from
it, and the texts the tests of that path share.  No device, no library: the decoder is checked against zlib where it is used."""
import zlib

import numpy as np

import deflate_craft as craft

WINDOW = 32768


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _decoder(lens):
    """canonical Huffman code of the lengths -> {(length, code): symbol}"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt, table = 0, [0] * 17, {}
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    for s, n in enumerate(lens):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


def _symbol(r, table):
    code, n = 0, 0
    while True:
        code = (code << 1) | r.take(1)
        n += 1
        if (n, code) in table:
            return table[(n, code)]
        assert n < 16, "no such code"


def sources(body):
    """raw deflate bytes -> (the text, src: for every byte of it the position it was copied from, -1 for a literal)"""
    r, out, src = _Bits(body), bytearray(), []
    fixed = None
    while True:
        last, kind = r.take(1), r.take(2)
        if kind == 0:
            r.pos = (r.pos + 7) & ~7
            n = r.take(16)
            assert r.take(16) == n ^ 0xFFFF
            at = r.pos >> 3
            out += body[at:at + n]
            src += [-1] * n
            r.pos += 8 * n
        else:
            assert kind in (1, 2)
            if kind == 1:
                fixed = fixed or (_decoder(craft.FIXED_LL), _decoder([5] * 30))
                ll, dd = fixed
            else:
                hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[craft.CL_ORDER[k]] = r.take(3)
                clt, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(r, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.take(2))
                    elif s == 17:
                        lens += [0] * (3 + r.take(3))
                    else:
                        lens += [0] * (11 + r.take(7))
                ll, dd = _decoder(lens[:hlit]), _decoder(lens[hlit:])
            while True:
                s = _symbol(r, ll)
                if s < 256:
                    out.append(s)
                    src.append(-1)
                elif s == 256:
                    break
                else:
                    n = craft.LEN_BASE[s - 257] + r.take(craft.LEN_EXTRA[s - 257])
                    d = _symbol(r, dd)
                    dist = craft.DIST_BASE[d] + r.take(craft.DIST_EXTRA[d])
                    for _ in range(n):
                        p = len(out)
                        out.append(out[p - dist])
                        src.append(p - dist)
        if last:
            return bytes(out), np.array(src, dtype=np.int64)


def out_window(text, src, a, b):
    """The out-window of the piece [a, b) of the text: entry i is the symbol WINDOW - i in front of b.  A position inside the piece
    is followed through its copies while they stay inside the piece: it ends at a literal of the piece (a byte) or at a
    position in front of a, which is a marker into the window in front of the piece - every copy reaches at most WINDOW back,
    so it lies in that window.  A position in front of a passes through as the marker of itself."""
    q = b - WINDOW + np.arange(WINDOW, dtype=np.int64)
    data = np.frombuffer(text, dtype=np.uint8)
    while True:
        inside = q >= a
        copied = inside & (src[np.where(inside, q, 0)] >= 0) if len(src) else inside & False
        if not copied.any():
            break
        q = np.where(copied, src[np.where(copied, q, 0)], q)
    # (a position in front of the text's first byte passes through like any other: nothing is there, and its marker says where)
    inside = q >= a
    byte = data[np.where(inside, q, 0)] if len(data) else np.zeros(WINDOW, dtype=np.uint8)
    return np.where(inside, byte.astype(np.uint16), (0x8000 | ((q - (a - WINDOW)) & 0x7FFF)).astype(np.uint16)).astype(np.uint16)


def windows_of(text, src, cuts):
    """cuts: ascending offsets 0 = cuts[0] <= ... <= cuts[-1] = len(text) -> the out-window of every piece, parts x WINDOW"""
    return np.stack([out_window(text, src, cuts[k], cuts[k + 1]) for k in range(len(cuts) - 1)])


def window_in_front(text, a, nothing):
    """the WINDOW bytes in front of text position a, `nothing` where the text has not begun"""
    w = np.full(WINDOW, nothing, dtype=np.uint16)
    have = min(a, WINDOW)
    if have:
        w[WINDOW - have:] = np.frombuffer(text[a - have:a], dtype=np.uint8)
    return w


def far_text(n_bytes, seed, names=40):
    """PAF lines of the reads r0 .. r39 with lengths 1000 + i (tests/test_gpu_ranks_compressed.py: NAMES40, LENS40) whose runs of
    records come back 20 000 to 32 768 bytes later: a block of lines, then blocks that repeat whole lines of the block in front
    of them from that far back - matches at the long distances, across whatever boundary falls between"""
    rng = np.random.default_rng(seed)
    lines, size, starts = [], 0, []

    def rec(a, b, k):
        return "r%d\t%d\t%d\t%d\t+\tr%d\t%d\t%d\t%d\t400\t%d\t255" % (a, 1000 + a, k % 90, 500 + k % 300, b, 1000 + b, k % 80, 480 + k % 200,
                                                                          450 + k % 50)

    k = 0
    while size < n_bytes:
        # a line from 20 000 .. 32 768 bytes back where there is one, else a new one
        want = size - int(rng.integers(20_000, WINDOW - 200))
        if want > 0 and rng.random() < 0.7:
            j = int(np.searchsorted(starts, want))
            line = lines[min(j, len(lines) - 1)]
        else:
            line = rec(int(rng.integers(0, names)), int(rng.integers(0, names)), int(rng.integers(0, 10_000)))
        starts.append(size)
        lines.append(line)
        size += len(line) + 1
        k += 1
    return ("\n".join(lines) + "\n").encode()


def deflate(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(text) + c.flush()
