"""CPU: the read-name table (rala_amd/csrc/name_table.h; rala::io::NameTable) as the device build of it relies on it - no
device here.  The hash has one definition: a vectorised numpy restatement is pinned to rala_hip_name_hash.  NameTable::adopt
takes over finished buckets.  The capacity rule.  And the premise tests/test_gpu_name_table.py rests on: the SET of occupied
slots and every answer are the same whatever the order of insertion - which slot holds what is the only freedom a parallel
build has.  A birthday search finds the colliding names that test feeds the device with."""
import ctypes
import os

import numpy as np
import pytest

from rala_amd import build, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT = 0xFFFFFFFFFFFFFFFF
ALPHABET = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)


def _lib():
    build.build_host()
    L = ctypes.CDLL(os.path.join(ROOT, "rala_amd", "host", "libassembly_graph.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.io_names_build.restype = vp
    L.io_names_build.argtypes = [vp, vp, u64, vp]
    L.io_names_adopt.restype = vp
    L.io_names_adopt.argtypes = [vp, u64, vp, u64]
    L.io_names_buckets.restype = u64
    L.io_names_buckets.argtypes = [vp]
    L.io_names_arena_bytes.restype = u64
    L.io_names_arena_bytes.argtypes = [vp]
    L.io_names_copy.argtypes = [vp, vp, vp]
    L.io_names_find.argtypes = [vp, vp, vp, u64, vp]
    L.io_names_hash.restype = u64
    L.io_names_hash.argtypes = [ctypes.c_char_p, u64]
    L.io_names_free.argtypes = [vp]
    return L


def _packed(names):
    blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
    return blob, np.array([len(s) for s in names], dtype=np.uint32)


class HostTable:
    """rala::io::NameTable through the shim: built from names (bytes, in id order; order: the order of insertion) or adopted"""

    def __init__(self, names=None, order=None, adopt=None):
        self.L = _lib()
        if adopt is not None:
            buckets, arena = adopt
            buckets = np.ascontiguousarray(buckets, dtype=np.uint32)
            arena = np.ascontiguousarray(arena, dtype=np.uint8)
            self.h = self.L.io_names_adopt(buckets.ctypes.data, buckets.shape[0], arena.ctypes.data if len(arena) else None, len(arena))
        else:
            blob, lens = _packed(names)
            if order is not None:
                order = np.ascontiguousarray(order, dtype=np.uint64)
                assert sorted(order.tolist()) == list(range(len(names)))
            self.h = self.L.io_names_build(blob.ctypes.data, lens.ctypes.data, len(names), order.ctypes.data if order is not None else None)

    def close(self):
        if self.h:
            self.L.io_names_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def find(self, queries):
        blob, lens = _packed(queries)
        out = np.zeros(len(queries), dtype=np.uint64)
        self.L.io_names_find(self.h, blob.ctypes.data, lens.ctypes.data, len(queries), out.ctypes.data)
        return out

    def table(self):
        """-> (buckets as (n_buckets, 8) uint32: hash32, id1, len, off, head; arena)"""
        buckets = np.zeros((int(self.L.io_names_buckets(self.h)), 8), dtype=np.uint32)
        arena = np.zeros(max(int(self.L.io_names_arena_bytes(self.h)), 1), dtype=np.uint8)
        self.L.io_names_copy(self.h, buckets.ctypes.data, arena.ctypes.data)
        return buckets, arena[:int(self.L.io_names_arena_bytes(self.h))]

    def occupied(self):
        return np.flatnonzero(self.table()[0][:, 1] != 0)


def np_hash(rows):
    """name_hash_with (name_table.h) restated over the rows of a (count, n) uint8 matrix: count names of n bytes -> uint64"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    count, n = rows.shape
    padded = np.zeros((count, (n + 7) // 8 * 8), dtype=np.uint8)
    padded[:, :n] = rows
    words = padded.view("<u8")
    u = np.uint64
    with np.errstate(over="ignore"):
        h = np.full(count, u(0x9E3779B97F4A7C15) ^ (u(n) * u(0xFF51AFD7ED558CCD)), dtype=np.uint64)
        for k in range(words.shape[1]):         # (full words, then the zero-padded rest: one more step of the same shape)
            h = (h ^ words[:, k]) * u(0xC2B2AE3D27D4EB4F)
            h ^= h >> u(29)
        h = h * u(0x165667B19E3779F9)
    return h ^ (h >> u(32))


def random_names(rng, count, n):
    """count names of n bytes over letters and digits, as a matrix"""
    return ALPHABET[rng.integers(0, len(ALPHABET), size=(count, n))]


_found = {}


def colliding_names(pool=4_000_000, seed=11):
    """A birthday search over `pool` random 8-byte names: names with equal hash32 (the high half of the hash, what a bucket
    keeps) and equal length.  -> dict: "same_home" / "adjacent_home": lists of (a, b) whose home slots in a table of 16 buckets
    are equal / next to each other (mod 16); "between": for the first same_home pair a third name of another hash32 with that
    home slot; "last_slot": names whose home is slot 15."""
    if "v" in _found:
        return _found["v"]
    rng = np.random.default_rng(seed)
    rows = np.unique(random_names(rng, pool, 8).view("<u8").ravel()).view(np.uint8).reshape(-1, 8)
    h = np_hash(rows)
    h32, home = h >> np.uint64(32), (h & np.uint64(15)).astype(np.int64)
    order = np.argsort(h32, kind="stable")
    eq = np.flatnonzero(h32[order][1:] == h32[order][:-1])
    a, b = order[eq], order[eq + 1]
    gap = (home[b] - home[a]) % 16
    name = lambda i: rows[i].tobytes()
    out = {"same_home": [(name(i), name(j)) for i, j in zip(a[gap == 0], b[gap == 0])],
           "adjacent_home": [(name(i), name(j)) if g == 1 else (name(j), name(i)) for i, j, g in zip(a, b, gap) if g in (1, 15)],
           "last_slot": [name(i) for i in np.flatnonzero(home == 15)[:3]], "between": None}
    if out["same_home"]:
        i = a[gap == 0][0]
        third = np.flatnonzero((home == home[i]) & (h32 != h32[i]))
        out["between"] = name(third[0])
    _found["v"] = out
    return out


def capacity(n):
    cap = 16
    while cap < 2 * n + 2:
        cap *= 2
    return cap


def test_numpy_hash_equals_the_one_definition():
    rng = np.random.default_rng(5)
    L = _lib()
    for n in list(range(0, 41)) + [1024]:
        rows = rng.integers(0, 256, size=(7, n), dtype=np.uint8)
        want = [hip.name_hash(rows[k].tobytes()) for k in range(len(rows))]
        assert np_hash(rows).tolist() == want, n
        # ... which is the host readers' as well
        assert [int(L.io_names_hash(rows[k].tobytes(), n)) for k in range(len(rows))] == want, n


def test_adopt_then_find_round_trips():
    rng = np.random.default_rng(6)
    names = [random_names(rng, 1, int(n))[0].tobytes() for n in rng.integers(1, 60, 500)]
    names += [names[3], names[77]]                      # (duplicates: the later id answers)
    built = HostTable(names)
    adopted = HostTable(adopt=built.table())
    queries = names + [s + b"x" for s in names[:50]] + [s[:-1] for s in names[:50]] + [b""]
    want = built.find(queries)
    assert adopted.find(queries).tolist() == want.tolist()
    assert want[3] == len(names) - 2 and want[77] == len(names) - 1 and want[-1] == ABSENT
    b0, a0 = built.table()
    b1, a1 = adopted.table()
    assert (b0 == b1).all() and a0.tobytes() == a1.tobytes()


@pytest.mark.parametrize("n", [0, 1, 6, 7, 8, 15, 16])
def test_capacity_rule(n):
    """the smallest power of two not below 2 n + 2, at least 16"""
    want = {0: 16, 1: 16, 6: 16, 7: 16, 8: 32, 15: 32, 16: 64}[n]
    assert capacity(n) == want
    t = HostTable([b"read%d" % i for i in range(n)])
    assert t.table()[0].shape[0] == want
    assert len(t.occupied()) == n
    assert t.find([b"read%d" % i for i in range(n + 1)]).tolist() == list(range(n)) + [ABSENT]


def shuffled_orders(names, rng, count):
    """orders of insertion in which, of every name, the LAST id comes behind its other ids (NameTable::build: the later one takes
    the name) - otherwise free"""
    last, groups = {}, {}
    for i, s in enumerate(names):
        last[s] = i
        groups.setdefault(s, []).append(i)
    out = []
    for _ in range(count):
        perm = rng.permutation(len(names)).tolist()
        place = {i: k for k, i in enumerate(perm)}
        # every name's last id changes places with whichever of its ids stands last
        for s, ids in groups.items():
            latest = max(ids, key=lambda i: place[i])
            if latest != last[s]:
                ka, kb = place[latest], place[last[s]]
                perm[ka], perm[kb] = perm[kb], perm[ka]
                place[latest], place[last[s]] = kb, ka
        out.append(perm)
    return out


def test_occupied_slots_and_answers_do_not_depend_on_the_order_of_insertion():
    """linear probing: which slots are taken is a function of the SET of names; which name sits where is not.  Crowded small
    tables (n = 7 of 16, 15 of 32), colliding names among them, and a larger one with duplicates."""
    rng = np.random.default_rng(7)
    found = colliding_names()
    sets = []
    a, b = found["same_home"][0]
    sets.append([a, found["between"], b] + [s for s in found["last_slot"]] + [b"z"])
    sets.append([random_names(rng, 1, 8)[0].tobytes() for _ in range(15)])
    big = [random_names(rng, 1, int(n))[0].tobytes() for n in rng.integers(1, 40, 3000)]
    big += [big[i] for i in rng.integers(0, 3000, 300)]
    sets.append(big)
    for names in sets:
        base = HostTable(names)
        queries = names + [s + b"!" for s in names[:200]] + [s[:-1] for s in names[:200]]
        want, slots = base.find(queries), base.occupied()
        assert len(slots) == len(set(names))
        moved = 0
        for order in shuffled_orders(names, rng, 6):
            t = HostTable(names, order=order)
            assert t.occupied().tolist() == slots.tolist()
            assert t.find(queries).tolist() == want.tolist()
            moved += int((t.table()[0][:, 1] != base.table()[0][:, 1]).any())
        assert moved, "no order moved a name: the test shows nothing"


def test_birthday_search_finds_colliding_names_for_the_device():
    found = colliding_names()
    assert len(found["same_home"]) >= 1 and len(found["adjacent_home"]) >= 1 and found["between"] is not None
    assert len(found["last_slot"]) == 3
    for a, b in found["same_home"][:5] + found["adjacent_home"][:5]:
        ha, hb = hip.name_hash(a), hip.name_hash(b)
        assert a != b and len(a) == len(b) == 8 and ha >> 32 == hb >> 32
        assert ((hb & 15) - (ha & 15)) % 16 in (0, 1)
    a, _ = found["same_home"][0]
    c = found["between"]
    assert hip.name_hash(c) & 15 == hip.name_hash(a) & 15 and hip.name_hash(c) >> 32 != hip.name_hash(a) >> 32
    assert all(hip.name_hash(s) & 15 == 15 for s in found["last_slot"])


def test_entry_points_are_exported_and_bound():
    L = hip.lib()
    for name in ("rala_hip_build_name_table", "rala_hip_get_name_table", "rala_hip_copy_name_table", "rala_hip_name_hash",
                 "rala_hip_get_name_table_info"):
        assert hasattr(L, name) and name in hip.SYMBOLS
    assert callable(hip.Context.build_name_table) and callable(hip.Context.get_name_table)
