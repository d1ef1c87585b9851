"""CPU: the two host functions of a gzip member taken by several ranks together (option gzip_in_pieces) - rala_hip_gzip_pieces,
which gives every part its run of the chain's jobs, and rala_hip_gzip_compose_windows, which makes the 32 768 bytes in front of
a part from the parts' out-windows.  The windows are checked against a model built from real streams (gzip_pieces_model: zlib's
streams decoded with every byte's source remembered, the text itself checked against zlib's)."""
import itertools
import os
import zlib

import numpy as np
import pytest

from rala_amd import hip

import gzip_pieces_model as model

W = model.WINDOW
NOTHING = hip.GZIP_NOTHING


@pytest.fixture(scope="module")
def streams():
    """a text of a few windows with matches up to 32 768 back, through zlib at levels 1 / 6 / 9 -> {level: (text, src)}"""
    text = model.far_text(150_000, 5)
    out = {}
    for level in (1, 6, 9):
        body = model.deflate(text, level)
        got, src = model.sources(body)
        assert got == text == zlib.decompressobj(-15).decompress(body)
        assert (src >= 0).sum() > len(text) // 2 and int((np.arange(len(text)) - src)[src >= 0].max()) > 30_000
        out[level] = (text, src)
    return out


def composed(windows, part):
    got, valid = hip.gzip_compose_windows(windows, part)
    return got, valid


def check_cuts(text, src, cuts):
    windows = model.windows_of(text, src, cuts)
    for part in range(len(cuts) - 1):
        got, valid = composed(windows, part)
        assert valid == 1, (cuts, part)
        want = model.window_in_front(text, cuts[part], NOTHING)
        assert (got == want).all(), (cuts, part, int(np.argmax(got != want)))


def test_the_header_names_the_code_and_it_is_neither_byte_nor_marker():
    assert 0x0100 <= NOTHING <= 0x7FFF
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rala_hip.h")
    assert "#define RALA_HIP_GZIP_NOTHING 0x%04X" % NOTHING in open(header).read()


@pytest.mark.parametrize("level", [1, 6, 9])
def test_windows_of_real_streams_cut_anywhere(streams, level):
    """1 - 9 pieces at arbitrary offsets: the composed window in front of every piece is the text's 32 768 bytes in front of it,
    nothing where the text has not begun"""
    text, src = streams[level]
    rng = np.random.default_rng(level)
    n = len(text)
    for parts in range(1, 10):
        inner = sorted(int(x) for x in rng.integers(0, n + 1, parts - 1))
        check_cuts(text, src, [0] + inner + [n])
    # the first boundary below one window, the others a window and more apart
    check_cuts(text, src, [0, 9_000, 50_001, 90_000, n])


def test_short_and_empty_pieces_compose_through_several_parts(streams):
    """pieces shorter than a window and empty ones: a part's window is made of the out-windows of several parts in front of it"""
    text, src = streams[6]
    n = len(text)
    check_cuts(text, src, [0, 0, 5_000, 5_000, 5_001, 12_000, 30_000, 30_000, 41_000, n])
    check_cuts(text, src, [0, 100_000, 100_000, 100_000, 100_700, 101_000, 131_000, n, n, n])
    # nothing but empty pieces in front: the window is nothing at all
    windows = model.windows_of(text, src, [0, 0, 0, n])
    for part in range(3):
        got, valid = composed(windows, part)
        assert valid == 1 and (got == NOTHING).all()


def test_identity_windows_pass_everything_through():
    """a part without text hands its in-window on: 0x8000 | i at entry i"""
    rng = np.random.default_rng(3)
    first = rng.integers(0, 256, W).astype(np.uint16)
    identity = (0x8000 | np.arange(W)).astype(np.uint16)
    windows = np.stack([first, identity, identity, identity])
    for part in (1, 2, 3):
        got, valid = composed(windows, part)
        assert valid == 1 and (got == first).all()
    got, valid = composed(windows, 0)
    assert valid == 1 and (got == NOTHING).all()
    # in front of the text identity hands nothing on
    got, valid = composed(np.stack([identity, identity]), 1)
    assert valid == 1 and (got == NOTHING).all()


def test_marker_zero_is_a_marker():
    """0x8000 | 0 names entry 0 of the window in front: it is not "nothing" """
    first = np.full(W, ord("a"), dtype=np.uint16)
    first[0] = ord("z")
    second = np.full(W, 0x8000, dtype=np.uint16)
    got, valid = composed(np.stack([first, second, second]), 2)
    assert valid == 1 and (got == ord("z")).all()
    # a shift by one: entry i is entry i + 1 of the window in front, the last one a byte
    shift = (0x8000 | (np.arange(W) + 1)).astype(np.uint16)
    shift[-1] = ord("q")
    got, valid = composed(np.stack([first, shift, shift]), 2)
    assert valid == 1 and got[-1] == ord("q") and (got[:-1] == ord("a")).all()


def test_a_marker_that_lands_on_nothing_is_refused():
    """the match that reaches in front of the text's first byte: nothing behind a byte"""
    # part 0 has 100 bytes of text and then copies from 200 back: 100 bytes in front of the text
    first = (0x8000 | ((np.arange(W) + 200) & 0x7FFF)).astype(np.uint16)           # passes its in-window through ...
    first[-200:-100] = ord("x")                                                    # ... then its own 100 bytes ...
    first[-100:] = (0x8000 | (W - 300 + np.arange(100))).astype(np.uint16)        # ... then what lay 200 in front of them
    got, valid = composed(np.stack([first, first]), 1)
    assert valid == 0
    assert (got[-200:-100] == ord("x")).all() and (got[-100:] == NOTHING).all()
    # the same part with bytes there is taken
    first[-100:] = ord("y")
    got, valid = composed(np.stack([first, first]), 1)
    assert valid == 1 and (got[:-200] == NOTHING).all()
    # a value that is neither a byte nor a marker
    bad = np.full(W, ord("a"), dtype=np.uint16)
    bad[77] = 0x0100
    assert composed(np.stack([bad, bad]), 1)[1] == 0
    bad[77] = NOTHING
    assert composed(np.stack([bad, bad]), 1)[1] == 0


def test_compose_windows_refuses_bad_arguments():
    L = hip.lib()
    w = np.zeros(W, dtype=np.uint16)
    import ctypes
    valid = ctypes.c_int32(0)
    assert L.rala_hip_gzip_compose_windows(w.ctypes.data, 1, 1, w.ctypes.data, ctypes.byref(valid)) != 0       # part >= parts
    assert L.rala_hip_gzip_compose_windows(None, 1, 0, w.ctypes.data, ctypes.byref(valid)) != 0
    assert L.rala_hip_gzip_compose_windows(w.ctypes.data, 1, 0, None, ctypes.byref(valid)) != 0


# ---- rala_hip_gzip_pieces -------------------------------------------------------------------------------------------------
DEFLATE_OFF, CHUNK = 10, 1024


def part_chunk(n_chunks, parts, k):
    """the first chunk of part k: n_chunks k / parts, chunk 0 always part 0's"""
    if k == 0:
        return 0
    if k >= parts:
        return n_chunks
    return min(n_chunks, max(1, n_chunks * k // parts))


def chunk_of(bit, n_chunks):
    return min((bit // 8 - DEFLATE_OFF) // CHUNK, n_chunks - 1)


def check_split(bits, n_chunks, parts):
    first = hip.gzip_pieces(bits, DEFLATE_OFF, CHUNK, n_chunks, parts)
    assert first is not None, (bits, n_chunks, parts)
    assert len(first) == parts + 1 and first[0] == 0 and first[-1] == len(bits)
    assert all(first[k] <= first[k + 1] for k in range(parts)), first             # contiguous, ascending, all jobs covered
    for k in range(parts):
        lo, hi = part_chunk(n_chunks, parts, k), part_chunk(n_chunks, parts, k + 1)
        for j in range(first[k], first[k + 1]):
            assert lo <= chunk_of(bits[j], n_chunks) < hi, (bits, n_chunks, parts, k, j)
    return first


def test_every_split_of_small_chains():
    """chains of 1 - 40 jobs over 1 - 9 parts: job 0 at the stream's first bit, the others at a bit of a chunk of their own"""
    rng = np.random.default_rng(9)
    seen_empty = seen_all_in_zero = 0
    for n_jobs, parts in itertools.product(range(1, 41), range(1, 10)):
        for n_chunks in (n_jobs, n_jobs + 3, 3 * n_jobs + 1, 64):
            if n_chunks < n_jobs:
                continue
            chunks = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n_chunks), n_jobs - 1, replace=False)) if n_jobs > 1 else [0]
            bits = [8 * DEFLATE_OFF] + [8 * (DEFLATE_OFF + c * CHUNK) + int(rng.integers(0, 8 * CHUNK)) for c in chunks[1:]]
            first = check_split(bits, n_chunks, parts)
            seen_empty += any(first[k] == first[k + 1] for k in range(parts))
            seen_all_in_zero += parts > 1 and first[1] == n_jobs
    assert seen_empty > 50 and seen_all_in_zero > 5


def test_parts_without_a_job_and_all_jobs_in_part_zero():
    # a stream of fixed or stored blocks: one job, whatever the number of chunks
    for parts in range(1, 10):
        for n_chunks in (1, 2, 7, 1000):
            assert check_split([8 * DEFLATE_OFF], n_chunks, parts) == [0] + [1] * parts
    # a file of one chunk over eight ranks; no job at all
    assert check_split([8 * DEFLATE_OFF + 3], 1, 8) == [0] + [1] * 8
    assert hip.gzip_pieces([], DEFLATE_OFF, CHUNK, 5, 4) == [0] * 5
    # jobs in the chunks of parts 0 and 3 alone
    bits = [8 * DEFLATE_OFF, 8 * (DEFLATE_OFF + CHUNK) + 5, 8 * (DEFLATE_OFF + 7 * CHUNK)]
    assert check_split(bits, 8, 4) == [0, 2, 2, 2, 3]
    # a start in the last, short chunk and one (never found there, but tolerated) behind it
    assert check_split([8 * DEFLATE_OFF, 8 * (DEFLATE_OFF + 9 * CHUNK), 8 * (DEFLATE_OFF + 50 * CHUNK)], 10, 2) == [0, 1, 3]


def test_pieces_refuses_what_is_no_chain():
    ok = [8 * DEFLATE_OFF, 8 * (DEFLATE_OFF + 3 * CHUNK)]
    assert hip.gzip_pieces(ok, DEFLATE_OFF, CHUNK, 8, 2) is not None
    assert hip.gzip_pieces(ok, DEFLATE_OFF, CHUNK, 8, 0) is None                            # no parts
    assert hip.gzip_pieces(ok[::-1], DEFLATE_OFF, CHUNK, 8, 2) is None                      # descending
    assert hip.gzip_pieces([ok[0], ok[0]], DEFLATE_OFF, CHUNK, 8, 2) is None                # not ascending
    assert hip.gzip_pieces(ok, DEFLATE_OFF, 0, 8, 2) is None
    assert hip.gzip_pieces(ok, DEFLATE_OFF, CHUNK, 0, 2) is None
    assert hip.gzip_pieces([8 * DEFLATE_OFF - 8], DEFLATE_OFF, CHUNK, 8, 2) is None         # in front of the deflate bytes
