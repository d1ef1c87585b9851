"""CPU: the tile algorithm of pile_rows_kernel.hip restated in NumPy - carry-in from the events in front of a tile, deltas of
the events inside it, a scan - against a direct Pile::add_layers loop (reference pile.cpp:274-297) on random events, coverage
that wraps mod 2^16 included.  Pins the tile size and the carry logic where no GPU is needed; and the new export's place in
header, library and Python binding (tests/test_abi.py compares the three)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_tile():
    text = open(os.path.join(ROOT, "rala_amd", "csrc", "kernels.h")).read()
    return int(re.search(r"constexpr uint32_t kRowsTile = (\d+);", text).group(1))


def add_layers(n, bounds):
    """the reference's loop, value by value: uint16 coverage counter, data_[i] += coverage between consecutive bounds"""
    row = np.zeros(n, dtype=np.uint16)
    cov, last = 0, 0
    for b in sorted(int(x) for x in bounds):
        pos = b >> 1
        if cov:
            for i in range(last, min(pos, n)):
                row[i] = (int(row[i]) + cov) & 0xFFFF
        last = pos
        cov = (cov - 1) & 0xFFFF if b & 1 else (cov + 1) & 0xFFFF
    return row


def rows_by_tiles(n, bounds, tile, sens=None):
    """what the kernel does: per tile the events in any order - in front of the tile into the carry, inside it into 32-bit
    deltas, behind it passed over; coverage = carry + inclusive scan of the deltas, cut to 16 bits; a second list of bounds
    (the sensitive ones) goes through the same loop"""
    events = np.concatenate([np.asarray(bounds, dtype=np.uint32), np.asarray(sens if sens is not None else [], dtype=np.uint32)])
    pos = (events >> 1).astype(np.int64)
    d = np.where(events & 1, -1, 1).astype(np.int32)
    row = np.zeros(n, dtype=np.uint16)
    for t0 in range(0, n, tile):
        carry = int(d[pos < t0].sum())          # begins minus ends in front of the tile
        delta = np.zeros(tile, dtype=np.int32)
        inside = (pos >= t0) & (pos < t0 + tile)
        np.add.at(delta, pos[inside] - t0, d[inside])
        cov = (carry + np.cumsum(delta, dtype=np.int64)) & 0xFFFF
        m = min(tile, n - t0)
        row[t0:t0 + m] = cov[:m].astype(np.uint16)
    return row


def random_bounds(rng, n, k, at_ends=True):
    b = rng.integers(0, n, size=k)
    e = np.minimum(n, b + rng.integers(1, max(2, n // 2), size=k))
    if at_ends and k >= 2:
        b[0], e[0] = 0, n               # events at position 0 and at len
        b[1], e[1] = 0, 1
    out = np.concatenate([b << 1, e << 1 | 1]).astype(np.uint32)
    rng.shuffle(out)                    # the kernel takes the events in any order
    return out


def test_tile_size_is_what_the_tests_assume():
    assert kernel_tile() == 8192


@pytest.mark.parametrize("tile", [8192, 64, 7])
def test_tiles_against_add_layers(tile):
    rng = np.random.default_rng(tile)
    T = tile
    for n in (1, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5):
        if n <= 0:
            continue
        for k in (0, 1, 3, 40):
            bounds = random_bounds(rng, n, k)
            want = add_layers(n, bounds)
            np.testing.assert_array_equal(rows_by_tiles(n, bounds, T), want)


def test_second_add_layers_on_top():
    rng = np.random.default_rng(5)
    n = 3 * 64 + 9
    primary, sens = random_bounds(rng, n, 30), random_bounds(rng, n, 7, at_ends=False)
    want = (add_layers(n, primary).astype(np.uint32) + add_layers(n, sens)) & 0xFFFF
    np.testing.assert_array_equal(rows_by_tiles(n, primary, 64, sens), want.astype(np.uint16))


def test_coverage_that_wraps():
    """ends in front of their begins (tests/wrapcase.py's rows): (0 - k) mod 2^16 across tile boundaries; and more than 2^16
    begins on one position"""
    n, T = 300, 64
    bounds = np.array([(10 << 1) | 1] * 3 + [(200 << 1)] * 3 + [(70 << 1), (130 << 1) | 1], dtype=np.uint32)
    want = add_layers(n, bounds)
    assert want[100] == 65536 - 3 + 1 and want[150] == 65536 - 3 and want[250] == 0
    np.testing.assert_array_equal(rows_by_tiles(n, bounds, T), want)
    many = np.array([(5 << 1)] * 70_000 + [(150 << 1) | 1] * 70_000, dtype=np.uint32)
    want = add_layers(n, many)
    assert want[100] == 70_000 - 65_536
    np.testing.assert_array_equal(rows_by_tiles(n, many, T), want)


def test_export_is_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "rala_hip.h")).read()
    assert re.search(r"int rala_hip_get_pile_rows_info\(rala_hip_ctx\* ctx, uint64_t\* resident_bytes, uint64_t\* rows_materialised\);", header)
    assert '"pile_rows"' in header and '"pile_rows_scratch_mb"' in header and "outside is 0" in header
    from rala_amd import hip
    assert "rala_hip_get_pile_rows_info" in hip.SYMBOLS
    assert hasattr(hip.Context, "pile_rows_info")
