"""GPU: the name table built on the device from the sequence index (rala_hip_build_name_table,
rala_amd/csrc/name_table_kernels.hip).  The verdict in every case is the host's NameTable - find on the table build makes from
the HOST reader's names of the same file: (a) the downloaded table, adopted, answers as it does for every name of the file, every
name with one byte changed, dropped or appended, and absent names; (b) the same set of occupied slots, the same capacity, the
same number of distinct names; (c) the device tokeniser gives the same columns for a PAF file over those names with the
device's table and with the host's.  Which name sits in which slot of a probe path is the one thing that may differ
(tests/test_name_table_cpu.py shows that on the host)."""
import ctypes

import numpy as np
import pytest

from rala_amd import hip

import test_name_table_cpu as nt
import test_sequences_cpu as seq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def fasta(names):
    return b"".join(b">" + s + b"\nACGT\n" for s in names)


def lengths_case():
    rng = np.random.default_rng(21)
    return [b""] + [nt.random_names(rng, 1, n)[0].tobytes() for n in (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 1024)]


def same_head_case():
    head = b"0123456789abcdef"
    return [head + b"A", head + b"B", head + b"A" + b"x" * 30 + b"1", head + b"A" + b"x" * 30 + b"2", head, head + b"A" * 7 + b"Q", head + b"A" * 7 + b"R"]


def duplicates_case(times, others):
    rng = np.random.default_rng(times)
    rest = [b"o%06d" % i for i in range(others)]
    names = rest + [b"the_one"] * times
    return [names[i] for i in rng.permutation(len(names))]


def random_case():
    rng = np.random.default_rng(22)
    rows = nt.random_names(rng, 200_000, 36)
    rows[rng.integers(0, 200_000, 2000)] = rows[rng.integers(0, 200_000, 2000)]         # 1 % duplicates
    return [r.tobytes() for r in rows]


def names_of(case):
    if case.startswith("reads_"):
        return [b"r%d" % i for i in range(int(case[6:]))]
    if case.startswith("collide") or case == "wraps_to_slot_0":
        found = nt.colliding_names()
        a, b = found["same_home"][0]
        p, q = found["adjacent_home"][0]
        names = {"collide_same_home": [a, b], "collide_adjacent": [p, q], "collide_third_between": [a, found["between"], b],
                 "wraps_to_slot_0": list(found["last_slot"])}[case.replace("_reversed", "")]
        return names[::-1] if case.endswith("_reversed") else names
    return {"lengths": lengths_case, "same_head": same_head_case, "twice": lambda: duplicates_case(2, 3),
            "wavefront_on_one_slot": lambda: [b"the_one"] * 64, "4096_times_among_4096": lambda: duplicates_case(4096, 4096),
            "random_200000": random_case}[case]()


CASES = ["reads_0", "reads_1", "reads_2", "reads_7", "reads_8", "lengths", "same_head", "collide_same_home", "collide_same_home_reversed",
         "collide_adjacent", "collide_adjacent_reversed", "collide_third_between", "collide_third_between_reversed", "wraps_to_slot_0",
         "twice", "wavefront_on_one_slot", "4096_times_among_4096", "random_200000"]


def mutations(names, rng, absent=1000):
    """every name with one byte changed, dropped and appended, and absent ones"""
    out = []
    at = rng.integers(0, 1 << 30, len(names)).tolist()
    for s, k in zip(names, at):
        k %= max(len(s), 1)
        if s:
            out.append(s[:k] + bytes([s[k] ^ 1]) + s[k + 1:])
            out.append(s[:k] + s[k + 1:])
        out.append(s + b"A")
    out += [b"absent/%d" % i for i in range(absent)]
    return out


def paf_text(names, rng, lines=2000):
    """12-column records over the names (none empty; one of 1024 bytes at most per line: the tokeniser's halo), unknown names and
    prefixes of known ones among them"""
    usable = [s for s in names if s]
    if not usable:
        usable = [b"nobody"]
    rows = []
    for k in range(lines):
        a, b = (usable[int(i)] for i in rng.integers(0, len(usable), 2))
        if len(a) + len(b) > 1100:
            b = b"short"
        kind = k % 7
        if kind == 3:
            a = a[:-1] or b"x"
        elif kind == 4 and len(b) < 1024:
            b = b + b"x"
        elif kind == 5:
            a = b"unknown%d" % k
        rows.append(b"\t".join([a, b"1000", b"%d" % (k % 500), b"%d" % (500 + k % 400), b"+-"[k & 1:(k & 1) + 1], b, b"1200", b"10", b"%d" % (300 + k % 50),
                                b"200", b"%d" % (400 + k % 9), b"255"]) + b"\n")
    return b"".join(rows)


def device_table(ctx, path, window=0):
    ctx.set_option("debug_sequence_window", window)
    irregular, index = ctx.index_sequences(path)
    assert irregular == 0
    n_buckets, n_distinct = ctx.build_name_table()
    buckets, arena = ctx.get_name_table()
    assert buckets.shape[0] == n_buckets
    return index, buckets, arena, n_distinct


def columns(ctx, paf):
    irregular, bad = ctx.set_overlaps_from_paf(paf)
    assert irregular == 0 and bad == -1
    return ctx.overlap_columns()


def check_against_host(ctx, tmp_path, names, rng, window=0):
    path = str(tmp_path / "reads.fasta")
    open(path, "wb").write(fasta(names))
    want_names = seq.host_read(path, False)["names"]            # (the HOST reader's names: the verdict's input)
    assert len(want_names) == len(names)
    host = nt.HostTable(want_names)
    index, buckets, arena, n_distinct = device_table(ctx, path, window)
    assert index["names"] == want_names
    # (b)
    host_buckets, host_arena = host.table()
    assert buckets.shape[0] == host_buckets.shape[0] == nt.capacity(len(names))
    assert np.flatnonzero(buckets[:, 1]).tolist() == host.occupied().tolist()
    assert n_distinct == len(host.occupied()) == len(set(want_names))
    assert (buckets[buckets[:, 1] == 0] == 0).all()
    info = ctx.name_table_info()
    assert info["names"] == len(names) and info["distinct"] == n_distinct and info["n_buckets"] == buckets.shape[0]
    assert info["longest_probe"] <= buckets.shape[0] and (info["longest_probe"] >= 1 or not names)
    # (a)
    adopted = nt.HostTable(adopt=(buckets, arena))
    queries = want_names + mutations(want_names, rng)
    want = host.find(queries)
    got = adopted.find(queries)
    assert got.tolist() == want.tolist()
    # (c) the tokeniser with the device's table, then with the host's (it wants reads: not over an empty file)
    if not names:
        return buckets, arena
    paf = str(tmp_path / "ovl.paf")
    open(paf, "wb").write(paf_text(want_names, rng))
    with_device = columns(ctx, paf)
    ctx.set_name_table(host_buckets, host_arena)
    with_host = columns(ctx, paf)
    assert len(with_host["a_id"]) == 2000
    for f in with_host:
        assert (with_device[f] == with_host[f]).all(), f
    if any(want_names):
        assert (with_host["a_id"] != 0xFFFFFFFF).any() and (with_host["a_id"] == 0xFFFFFFFF).any()
    return buckets, arena


@pytest.mark.parametrize("case", CASES)
def test_device_table_answers_as_the_host_table(ctx, tmp_path, case):
    names = names_of(case)
    rng = np.random.default_rng(len(names))
    buckets, arena = check_against_host(ctx, tmp_path, names, rng)
    # the ids the buckets hold: of every name its LAST record
    last = {s: i for i, s in enumerate(names)}
    assert sorted(buckets[:, 1][buckets[:, 1] != 0].tolist()) == sorted(i + 1 for i in last.values())
    if case == "wraps_to_slot_0":
        assert buckets[15, 1] != 0 and buckets[0, 1] != 0 and buckets[1, 1] != 0
    if case in ("wavefront_on_one_slot", "4096_times_among_4096", "twice"):
        assert nt.HostTable(adopt=(buckets, arena)).find([b"the_one"])[0] == last[b"the_one"]


def test_windows_of_one_byte_give_the_one_window_table(ctx, tmp_path):
    names = [b"w%d" % i for i in range(6)] + [b"w1", b"a_longer_name_than_16_bytes"]
    rng = np.random.default_rng(1)
    assert len(fasta(names)) < 200
    one, _ = check_against_host(ctx, tmp_path, names, rng)
    many, _ = check_against_host(ctx, tmp_path, names, rng, window=1)
    ctx.set_option("debug_sequence_window", 0)
    # (slots may hold other names of a path; hash, length and the set of ids may not differ)
    assert sorted(map(tuple, one[:, :3].tolist())) == sorted(map(tuple, many[:, :3].tolist()))


def test_second_build_replaces_the_first(ctx, tmp_path):
    first, second = [b"first%d" % i for i in range(40)], [b"second%d" % i for i in range(9)]
    for k, names in enumerate((first, second)):
        path = str(tmp_path / ("reads%d.fasta" % k))
        open(path, "wb").write(fasta(names))
        _, buckets, arena, n_distinct = device_table(ctx, path)
        assert n_distinct == len(names)
    assert buckets.shape[0] == 32
    adopted = nt.HostTable(adopt=(buckets, arena))
    assert adopted.find(second).tolist() == list(range(9))
    assert (adopted.find(first) == nt.ABSENT).all()


def test_build_without_an_index_is_refused_and_leaves_the_table(tmp_path):
    c = hip.Context(0)
    try:
        host = nt.HostTable([b"kept%d" % i for i in range(5)])
        buckets, arena = host.table()
        nb, nd = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert c.L.rala_hip_build_name_table(c.h, ctypes.byref(nb), ctypes.byref(nd)) == -2        # RALA_HIP_EINVAL
        assert c.L.rala_hip_get_name_table(c.h, None, None, ctypes.byref(nb), ctypes.byref(nd)) == -2   # (nothing installed yet)
        c.set_name_table(buckets, arena)
        assert c.L.rala_hip_build_name_table(c.h, ctypes.byref(nb), ctypes.byref(nd)) == -2
        assert nb.value == 0 and nd.value == 0
        got_buckets, got_arena = c.get_name_table()
        assert (got_buckets == buckets).all() and got_arena.tobytes() == arena.tobytes()
    finally:
        c.close()


def test_copy_to_a_second_context_outlives_the_source_index(ctx, tmp_path):
    names = [b"copied%d" % i for i in range(100)] + [b"a_name_of_more_than_16_bytes_%d" % i for i in range(20)]
    path = str(tmp_path / "reads.fasta")
    open(path, "wb").write(fasta(names))
    _, buckets, arena, _ = device_table(ctx, path)
    other = hip.Context(0)
    try:
        other.copy_name_table_from(ctx)
        # the source indexes another file and builds another table: the copy is its own
        path2 = str(tmp_path / "other.fasta")
        open(path2, "wb").write(fasta([b"elsewhere%d" % i for i in range(300)]))
        device_table(ctx, path2)
        got_buckets, got_arena = other.get_name_table()
        assert (got_buckets == buckets).all() and got_arena.tobytes() == arena.tobytes()
        # ... and the tokeniser of the second context finds the names in it
        other.set_reads(np.full(len(names), 1200, dtype=np.uint32))
        paf = str(tmp_path / "ovl.paf")
        open(paf, "wb").write(paf_text(names, np.random.default_rng(3)))
        got = columns(other, paf)
        other.set_name_table(*nt.HostTable(names).table())
        want = columns(other, paf)
        for f in want:
            assert (got[f] == want[f]).all(), f
        assert (want["a_id"] != 0xFFFFFFFF).any()
    finally:
        other.close()
