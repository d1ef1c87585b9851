"""CPU: the host side of the windowed gzip inflater and of the device slicer - the chaining of the windows' CRC registers
(rala_hip_crc32_chain: no device) against zlib, and the exports and bindings of the new entry points."""
import zlib

import numpy as np
import pytest

from rala_amd import hip


def register(piece):
    """the CRC register of a piece started from zero, no final inversion (the register is linear in its start value)"""
    return (zlib.crc32(piece) ^ zlib.crc32(bytes(len(piece)))) & 0xFFFFFFFF


@pytest.mark.parametrize("seed", range(6))
def test_crc32_chain_equals_zlib_for_random_splits(seed):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, int(rng.integers(1, 200_000)), dtype=np.uint8).tobytes()
    # cuts anywhere - no piece a multiple of the resolve pass's 16 KB segment on purpose - with empty pieces and pieces of one byte
    cuts = sorted(rng.integers(0, len(data) + 1, int(rng.integers(0, 40))).tolist())
    cuts = [0] + cuts + [c for c in cuts[:3]] + [min(c + 1, len(data)) for c in cuts[:3]] + [len(data)]
    cuts = sorted(cuts)
    pieces = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert b"".join(pieces) == data
    assert any(len(p) == 0 for p in pieces) or len(cuts) == 2
    got = hip.crc32_chain([register(p) for p in pieces], [len(p) for p in pieces])
    assert got == zlib.crc32(data) & 0xFFFFFFFF


def test_crc32_chain_edge_cases():
    assert hip.crc32_chain([], []) == zlib.crc32(b"")
    assert hip.crc32_chain([0, 0, 0], [0, 0, 0]) == zlib.crc32(b"")
    one = b"\x00"
    assert hip.crc32_chain([register(one)], [1]) == zlib.crc32(one)
    data = bytes(range(256)) * 300
    pieces = [data[i:i + 1] for i in range(50)] + [data[50:16384], data[16384:16385], data[16385:]]
    assert hip.crc32_chain([register(p) for p in pieces], [len(p) for p in pieces]) == zlib.crc32(data)
    # a piece of more than 4 GB of zeros in front (its register is zero): the length is 64 bits wide
    big = (1 << 32) + 5
    tail = b"tail"
    got = hip.crc32_chain([0, register(tail)], [big, len(tail)])
    crc = 0
    for _ in range(big >> 24):
        crc = zlib.crc32(bytes(1 << 24), crc)
    crc = zlib.crc32(tail, zlib.crc32(bytes(big & ((1 << 24) - 1)), crc))
    assert got == crc & 0xFFFFFFFF


def test_new_entry_points_are_exported_and_bound():
    L = hip.lib()
    for name in ("rala_hip_slice_sequences", "rala_hip_get_sequence_slice_info", "rala_hip_crc32_chain"):
        assert hasattr(L, name) and name in hip.SYMBOLS
    assert len(L.rala_hip_slice_sequences.argtypes) == 8
    assert len(L.rala_hip_crc32_chain.argtypes) == 3
    for method in ("slice_sequences", "sequence_slice_info", "gzip_timings"):
        assert callable(getattr(hip.Context, method))
    assert callable(hip.crc32_chain)
    assert [n for n, _ in hip.SequenceSliceInfo._fields_][:3] == ["windows", "max_window_text_bytes", "bases"]
