"""The cases of tests/compcase.py do what they were designed to do, shown with the oracle alone (no device).

These are conditions on the inputs, not measurements: tests/test_gpu_component_medians.py can only fail for a wrong component
median if, in the oracle, every component's two probes sit on either side of exactly the designed median.
"""
import numpy as np
import pytest

import compcase
import parity


@pytest.fixture(params=sorted(compcase.CASES))
def built(request):
    case = compcase.case(request.param)
    return case, parity.crafted_stages(case)


def _components(n, a, b, value):
    """union-find and a sort in plain numpy: {smallest member: (members, element at size // 2 of the sorted values)}"""
    parent = np.arange(n)

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = root(x), root(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    touched = np.zeros(n, dtype=bool)
    touched[a] = touched[b] = True
    groups = {}
    for r in np.nonzero(touched)[0].tolist():
        groups.setdefault(root(r), []).append(r)
    return {k: (v, int(np.sort(value[v])[len(v) // 2])) for k, v in groups.items()}


def test_usable_medians():
    """the probe arithmetic, in the kernels' doubles: 25 * 1.84 is 46 on paper and a hair above it in double"""
    assert compcase.LOW_MEDIANS == [12, 23] and len(compcase.HIGH_MEDIANS) > 40
    for M in compcase.LOW_MEDIANS + compcase.HIGH_MEDIANS + [253, 264]:
        a = compcase.probe_minimum(M)
        assert a * 1.84 <= M and not (a * 1.84 <= M - 1) and not ((a + 1) * 1.84 <= M) and (a + 1) * 1.84 <= M + 1
    assert compcase.probe_minimum(13) is None and compcase.probe_minimum(255) is None


def test_every_edge_has_its_case():
    names = set(compcase.CASES)
    assert {"sizes_interleaved", "sizes_contiguous", "high_byte", "ties", "split", "large", "shape_chain", "shape_chain_permuted",
            "shape_star", "shape_cliques", "shape_third"} <= names
    for name in ("sizes_interleaved", "sizes_contiguous"):
        case = compcase.case(name)
        assert {c.size for c in case.comps} == set(compcase.SIZES)
        # the components' stretches of the select's value array, in root order, start on every residue mod 8 - the large ones too
        order = sorted(case.comps, key=lambda c: min(c.members))
        starts = np.concatenate(([0], np.cumsum([c.size for c in order])[:-1]))
        assert set((starts % 8).tolist()) == set(range(8))
        assert len({int(s) % 8 for s, c in zip(starts, order) if c.size > 64}) >= 6
        # neighbours in that order: a low median beside a high one, far more than a probe's step apart
        for x, y in zip(order[:-1], order[1:]):
            assert abs(x.M - y.M) > 250 or 2 in (x.size, y.size), (x.name, y.name)
    inter, contig = compcase.case("sizes_interleaved"), compcase.case("sizes_contiguous")
    big = [c for c in inter.comps if c.size == 1025][0]
    assert len({m // 256 for m in big.members}) > 10 and len({inter.comp_of[r] for r in range(512, 576)}) > 8
    big = [c for c in contig.comps if c.size == 1025][0]
    assert max(big.members) - min(big.members) < 1025 + 40
    # even sizes: the lower median is out of a probe's reach
    for c in inter.comps:
        if c.size % 2 == 0 and c.size > 2:
            v = sorted(c.values)
            assert v[c.size // 2] - v[c.size // 2 - 1] >= 3
    large = compcase.case(compcase.LARGE)
    assert max(c.size for c in large.comps) > 32768 and len(large.comps) > 200
    high = {c.name: c for c in compcase.case("high_byte").comps}
    for s in (100, 101, 640):
        v = sorted(high["last_of_byte0_%d" % s].values)
        assert v[s // 2] == 253 and v[s // 2 + 1] >= 256 and v[0] < 253
        v = sorted(high["first_of_byte1_%d" % s].values)
        assert v[s // 2] == 264 and v[s // 2 - 1] == 255
    assert len(set(high["all_equal_130"].values)) == 1 and len(set(high["all_distinct_200"].values)) == 200
    assert min(high["above_4096"].values) > 4096
    for c in compcase.case("ties").comps:
        assert c.size <= 65 and c.values.count(c.M) >= c.size // 2 - 1


def test_loose_reads_are_where_they_matter():
    case = compcase.case("sizes_interleaved")
    assert case.kind[0] == 2
    live = np.nonzero(case.kind != 2)[0]
    for rank in (0, 64, 256, 1024):
        assert case.kind[live[rank]] == 1, rank
    assert (live != np.arange(len(live))).any()


def test_designed_state_is_what_the_oracle_finds(built):
    case, st = built
    alive = case.kind != 2
    assert (st["piles0"]["alive"] == alive).all()
    assert (st["valid"] == 1).all()
    # a live read's valid region is its whole row, a dead one has none
    assert (st["piles0"]["begin"] == 0).all() and (st["piles0"]["end"] == np.where(alive, case.read_len, 0)).all()
    # the pile medians are the designed ones
    assert (st["piles0"]["median"][alive] == case.value[alive]).all()
    assert (st["piles0"]["p10"][alive] == case.value[alive]).all()
    # exactly the designed pit on every probe (and the bridge), none elsewhere; no hills at all
    offs, pairs = compcase.designed_pits(case)
    assert (st["pits0"][0] == offs).all() and (st["pits0"][1] == pairs).all()
    assert len(st["hills0"][1]) == 0
    aux = compcase.pit_minima(case, offs, pairs)
    for r, (at, dip) in case.pit.items():
        assert aux[int(offs[r])] == dip


def test_components_and_medians_by_union_find(built):
    case, st = built
    src = st["ov_pass2"]["src"].astype(np.int64)
    assert len(st["int_pass2"]["src"]) == 0
    # the second pass kept every overlap between two live reads, as a dovetail
    a, b = case.overlaps.a_id[src].astype(np.int64), case.overlaps.b_id[src].astype(np.int64)
    live_pair = (case.kind[case.overlaps.a_id] != 2) & (case.kind[case.overlaps.b_id] != 2)
    assert (np.nonzero(live_pair)[0] == src).all()
    assert (st["ov_pass2"]["type"] == 3).all()
    found = _components(case.n_reads, a, b, case.value.astype(np.int64))
    assert len(found) == len(case.comps)
    for c in case.comps:
        members, M = found[min(c.members)]
        assert members == sorted(c.members), c.name
        assert M == c.M, (c.name, M, c.M)
    touched = np.zeros(case.n_reads, dtype=bool)
    touched[a] = touched[b] = True
    assert not touched[case.kind != 0].any() and touched[case.kind == 0].all()


def test_probes_decide(built):
    case, st = built
    p0, p2 = st["piles0"], st["piles2"]
    shrunk = (p0["begin"] != p2["begin"]) | (p0["end"] != p2["end"])
    wanted = np.zeros(case.n_reads, dtype=bool)
    for c in case.comps:
        assert "lower" in c.probes and "upper" in c.probes, c.name
        lo, up = c.probes["lower"], c.probes["upper"]
        assert case.pit[lo][1] == c.a and case.pit[up][1] == c.a + 1
        assert compcase.chimeric(c.a, c.M) and not compcase.chimeric(c.a, c.M - 1), c.name
        assert not compcase.chimeric(c.a + 1, c.M) and compcase.chimeric(c.a + 1, c.M + 1), c.name
        assert p2["alive"][lo] and p2["alive"][up], c.name
        assert shrunk[lo], "%s: the lower probe is whole" % c.name
        assert not shrunk[up], "%s: the upper probe is broken" % c.name
        wanted[lo] = True
        for role in ("second-tier lower", "bridge"):
            if role in c.probes:
                assert shrunk[c.probes[role]], "%s: the %s is whole" % (c.name, role)
                wanted[c.probes[role]] = True
        if "second-tier upper" in c.probes:
            assert not shrunk[c.probes["second-tier upper"]], c.name
    # nothing else moves, and nobody dies after the second pass
    assert (shrunk == wanted).all()
    assert (p2["alive"] == p0["alive"]).all()


def test_the_split_happens():
    case = compcase.case("split")
    st = parity.crafted_stages(case)
    c = [c for c in case.comps if c.tiers][0]
    (_, left, M1), (_, right, M2) = c.tiers
    assert M2 < c.M < M1
    src = st["ov"]["src"].astype(np.int64)
    a, b = case.overlaps.a_id[src].astype(np.int64), case.overlaps.b_id[src].astype(np.int64)
    found = _components(case.n_reads, a, b, case.value.astype(np.int64))
    assert found[min(left)] == (sorted(left), M1) and found[min(right)] == (sorted(right), M2)
    a1 = case.pit[c.probes["second-tier lower"]][1]
    assert not compcase.chimeric(a1, c.M) and compcase.chimeric(a1, M1) and not compcase.chimeric(a1, M1 - 1)
    assert not compcase.chimeric(a1 + 1, M1) and case.pit[c.probes["second-tier upper"]][1] == a1 + 1
