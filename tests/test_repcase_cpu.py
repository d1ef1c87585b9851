"""The cases of tests/repcase.py do what they were designed to do, shown with the oracle alone (no device).

These are conditions on the inputs, not measurements: tests/test_gpu_repeats.py can only fail for a wrong compare in the
sensitive pass if some case sits on that compare.  So the model of repcase.py - which names every decision it takes - has to
agree with the oracle on every case, and the census of its decisions over all cases has to have every decision on every side,
the ones the builder places by geometry with a margin of 0 or 1.  `census_text()` is what profiles/r18_repcase_census.txt holds.
"""
import os

import numpy as np
import pytest

from oracle import oracle as om
from oracle.oracle import Oracle

import repcase

CENSUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r18_repcase_census.txt")
BACKENDS = [False] + ([True] if om.have_ref() else [])


def _cases():
    """(layer, name, decisions) of every case: a call of Layer A, a read of a Layer B set"""
    for c in repcase.layer_a().calls:
        yield "A", c.name, c.log
    for name in sorted(repcase.BASES):
        cs = repcase.case_set(name)
        for r in sorted(cs.trace.log):
            yield "B", "%s/%d" % (name, r), cs.trace.log[r]


def census(layers="AB"):
    """{(decision, side): (number of cases, smallest margin)}"""
    seen = {}
    for layer, _, log in _cases():
        if layer not in layers:
            continue
        for key in {(d, s) for d, s, m in log}:
            n, low = seen.get(key, (0, None))
            m = min(m for d, s, m in log if (d, s) == key)
            seen[key] = (n + 1, m if low is None else min(low, m))
    return seen


def census_text():
    lines = ["# decision | side | cases | smallest margin    (tests/test_repcase_cpu.py::census_text)"]
    seen = census()
    for d in repcase.SIDES:
        for s in repcase.SIDES[d]:
            n, m = seen.get((d, s), (0, None))
            lines.append("%s | %s | %d | %s" % (d, s, n, "-" if m is None else m))
    return "\n".join(lines) + "\n"


# ---- Layer A -------------------------------------------------------------------------------------------------------------------
def test_layer_a_rows_are_what_initialize_leaves():
    """every value was designed in integers: the oracle's row after initialize is the designed one, the region [15, length - 15)"""
    A = repcase.layer_a()
    o = Oracle(A.read_len, A.overlaps, n_threads=8)
    assert o.initialize() == 0
    p = o.piles()
    for c in A.calls:
        assert p["alive"][c.read] and (p["begin"][c.read], p["end"][c.read]) == (repcase.kEdge, len(c.row) - repcase.kEdge), c.name
        assert (o.pile_data(c.read) == c.row).all(), c.name
        assert c.begin <= c.end <= len(c.row)


@pytest.mark.parametrize("ref", BACKENDS)
def test_layer_a_model_is_the_oracle(ref):
    for c in repcase.layer_a().calls:
        hills, flags = repcase.oracle_call(c, ref)
        assert hills == c.hills, "%s: oracle %s, model %s\n%s" % (c.name, hills, c.hills, c.log)
        assert not any(flags)


def test_layer_a_shapes():
    calls = {c.name: c for c in repcase.layer_a().calls}
    assert len(calls) == len(repcase.layer_a().calls)
    assert calls["between the slopes at 14 (peak value 14)"].hills == [] and calls["between the slopes at 15 (peak value 14)"].hills
    assert calls["between the slopes at 14 (peak value 14), mirrored"].hills == []
    assert calls["between the slopes at 15 (peak value 14), mirrored"].hills
    assert calls["plateau at 14 over floor 6, dataset median 10"].hills == []
    assert calls["plateau at 15 over floor 6, dataset median 10"].hills
    gaps = [c for n, c in calls.items() if n.startswith("two plateaus")]
    assert sorted(len(c.hills) for c in gaps) == [1, 2]
    wide = [c for n, c in calls.items() if n.startswith("wide plateau")]
    assert sorted(len(c.hills) for c in wide) == [0, 1] and abs(wide[0].end - wide[1].end) == 1
    # the switch: dataset medians on either side of median / 1.42, p10 below, at and above them
    for p10 in (14, 8, 21):
        taken = [dict((d, s) for d, s, m in calls["median 21, p10 %d, dataset median %d" % (p10, dm)].log)[repcase.MEDIAN_SWITCH]
                 for dm in (12, 13, 14, 15, 16)]
        assert taken == ["taken"] * 3 + ["not"] * 2
    # 1.42 * 50 is 71.0 in double: a median of 71 is not above it
    assert (repcase.MEDIAN_SWITCH, "not", 0) in calls["median 71, dataset median 50"].log
    assert 1.42 * 50 == 71.0
    # many pairs and a merge whose outcome depends on the order
    assert sum(1 for d in calls["staircase up"].log if d[0] == repcase.MERGE) >= 3


# ---- Layer B -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", BACKENDS)
@pytest.mark.parametrize("name", sorted(repcase.BASES))
def test_layer_b_model_is_the_oracle(name, ref):
    cs = repcase.case_set(name)
    if ref:
        st, t = repcase.sensitive_pass(cs.ds, cs.sens, ref=True)
        assert (st["rep"][1] == cs.st["rep"][1]).all() and (st["flags"] == cs.st["flags"]).all()
    else:
        st, t = cs.st, cs.trace
    assert repcase.verdict(st, t) is None, repcase.verdict(st, t)


@pytest.mark.parametrize("name", sorted(repcase.BASES))
def test_layer_b_targets(name):
    cs = repcase.case_set(name)
    assert cs.missed == [], "roles without a target: %s" % cs.missed
    assert 4 <= len(cs.targets) <= repcase.kMaxTargets and len(set(cs.targets)) == len(cs.targets)
    p, front = cs.st["piles"], cs.st["front"]
    offs = cs.st["rep"][0]
    in_component = set(front.ov["a_id"].tolist()) | set(front.ov["b_id"].tolist())
    for r in cs.targets:
        assert p["alive"][r] and r in in_component and int(p["end"][r]) - int(p["begin"][r]) > 8000, r
        assert offs[r + 1] > offs[r], "no hill on target %d (%s)" % (r, cs.roles[r])
    # the sets that had no hill at all have them on at least four targets
    if name != "cap512_cap1024":
        gen = repcase.Builder(name).st
        assert len(gen["rep"][1]) == 0
        assert sum(1 for r in cs.targets if offs[r + 1] > offs[r]) >= 4


def _has(cs, r, decision, side, margin=None):
    return any(d == decision and s == side and (margin is None or m == margin) for d, s, m in cs.trace.log[r])


def _flags(cs, r):
    offs = cs.st["rep"][0]
    return cs.st["flags"][int(offs[r]):int(offs[r + 1])].tolist()


def test_layer_b_roles_are_what_the_oracle_finds():
    """the verdict on every case is the oracle's: its flags, and (the model being the oracle) the decision the role names"""
    R = repcase
    seen, below = set(), False
    for name in sorted(R.BASES):
        cs = R.case_set(name)
        for r in cs.targets:
            role, flags = cs.roles[r], _flags(cs, r)
            seen.add(role.split(" (")[0])
            if role.startswith(("left hill", "right hill")):
                left = role.startswith("left")
                bridge, klass = (R.BRIDGE_LEFT, "left") if left else (R.BRIDGE_RIGHT, "right")
                assert len(flags) == 1 and _has(cs, r, R.CLASS, klass), (name, r, role)
                if "exact" in role:
                    # the designed dovetail alone bridges it, with not a base to spare
                    bridged = [m for d, s_, m in cs.trace.log[r] if d == bridge and s_ == "bridged"]
                    assert flags == [1] and bridged == [0], (name, r, role, bridged)
                    assert _has(cs, r, R.EDGE_LEFT, "left", 0) if left else _has(cs, r, R.EDGE_RIGHT, "right", 0), (name, r, role)
                elif "bridged" in role:
                    side, fuzz = role.split(", ")[2][0], int(role[-3:])
                    f = {("left", "a"): R.FILTER_LEFT_A, ("left", "b"): R.FILTER_LEFT_B, ("right", "a"): R.FILTER_RIGHT_A,
                         ("right", "b"): R.FILTER_RIGHT_B}[(klass, side)]
                    assert flags == [1] and _has(cs, r, bridge, "bridged", 0), (name, r, role)
                    assert _has(cs, r, f, "kept" if fuzz == 420 else "removed", 0), (name, r, role)
                elif "short" in role:
                    assert flags == [0] and _has(cs, r, bridge, "short", 0) and _has(cs, r, R.UNBRIDGED, "kept"), (name, r, role)
                elif "near tie" in role:
                    assert flags == [1] and _has(cs, r, R.TIE, "apart", 0), (name, r, role)
                else:
                    assert flags == [0] and _has(cs, r, R.TIE, "tie") and _has(cs, r, R.UNBRIDGED, "kept"), (name, r, role)
                    if "the larger is p10" in role:
                        assert _has(cs, r, R.MEDIAN_SWITCH, "taken") and _has(cs, r, R.MAX_OPERAND, "p10"), (name, r, role)
            elif role.startswith("inner plateau"):
                assert len(flags) == 1 and _has(cs, r, R.CLASS, "neither"), (name, r, role)
                if "first" in role:
                    assert _has(cs, r, R.EDGE_LEFT, "not", 0), (name, r, role)
                if "second" in role:
                    assert _has(cs, r, R.EDGE_RIGHT, "not", 0), (name, r, role)
            elif role.startswith("two plateaus"):
                assert len(flags) == (1 if "accepted" in role else 2), (name, r, role)
                assert _has(cs, r, R.MERGE, "absorbed" if "accepted" in role else "apart"), (name, r, role)
            elif role.startswith("left and right"):
                assert len(flags) == 1 and _has(cs, r, R.CLASS, "both"), (name, r, role)
            elif role.startswith("the peak test"):
                assert flags == [0] and _has(cs, r, R.PEAK, "none"), (name, r, role)
            elif role.startswith("median above"):
                assert _has(cs, r, R.MEDIAN_SWITCH, "taken") and _has(cs, r, R.MAX_OPERAND, role.split()[-1]), (name, r, role)
            else:
                assert role.startswith("plateau in the smallest component"), role
                assert cs.st["comp_size"][r] == min(cs.st["comp_size"].values())
        below = below or any(_has(cs, r, R.MEDIAN_SWITCH, "not") for r in cs.targets)
    assert below, "no target stays below the switch"
    want = {"inner plateau, first at the left edge", "inner plateau, second at the right edge", "two plateaus, the outer pair accepted", "two plateaus, the outer pair refused",
            "left and right at once", "plateau in the smallest component",
            "median above 1.42 * component median, the larger is dm",
            "right hill, tie, median above 1.42 * component median, the larger is p10",
            "the peak test refuses a pair whose larger end is w_first"}
    want |= {"%s hill, %s" % (k, v) for k in ("left", "right") for v in ("exact", "short")} | {"left hill, tie"} | {"left hill, near tie"}
    want |= {"left hill, bridged, %s side at +%d" % (s, z) for s in "ab" for z in (419, 420)}
    want |= {"right hill, bridged, %s side at -%d" % (s, z) for s in "ab" for z in (419, 420)}
    assert want <= seen, sorted(want - seen)


# ---- every placed decision shows ------------------------------------------------------------------------------------------------
TWEAKS = [(d, step) for d in repcase.PLACED for step in (1, -1)] + [("0.336", 0.335), ("0.336", 0.337), ("peak end", 1)]


def _noticed(layers="AB"):
    """the first case on which the model as repcase.TWEAK has it differs from the oracle, or None"""
    for c in repcase.layer_a().calls if "A" in layers else ():
        if c.model([]) != c.hills:
            return c.name
    for name in () if layers == "A" else ("cap2048", "cap512_cap1024", "position"):
        cs = repcase.case_set(name)
        if repcase.verdict(cs.st, cs.st["again"]()) is not None:
            return name
    return None


@pytest.mark.parametrize("decision,step", TWEAKS, ids=["%s %+g" % t for t in TWEAKS])
def test_a_model_wrong_by_one_differs_from_the_oracle(decision, step):
    """margin 0 on both sides says that the cases reach a compare; this says that its outcome shows: a model whose compare is
    off by one unit in either direction (or whose 0.336 is 0.335 / 0.337) gives other hills, flags or overlaps than the oracle"""
    assert _noticed() is None
    repcase.TWEAK[decision] = step
    try:
        where = _noticed()
    finally:
        repcase.TWEAK.clear()
    assert where is not None, "no case notices %r moved by %+g" % (decision, step)


def test_layer_b_alone_notices_the_peak_taken_from_one_end():
    """the run-space kernels see Layer B only: there too the peak test refuses a pair, and the pair's larger end is w_first"""
    b = census("B")
    assert (repcase.PEAK, "none") in b and (repcase.PEAK, "found") in b
    repcase.TWEAK["peak end"] = True
    try:
        where = _noticed("B")
    finally:
        repcase.TWEAK.clear()
    assert where == "cap512_cap1024", where


def test_tiers():
    """every designed target starts in the kernel its set is named for, by the rule of sens_split_kernel: reads of up to 16384
    bases with at most 510 / 1022 / 2046 events - two per primary record the read is in, two per sensitive record on it -
    go to the cap-512 / cap-1024 / cap-2048 run-space kernel, the others to position space"""
    for name in sorted(repcase.BASES):
        cs = repcase.case_set(name)
        ov, sens = cs.ds.overlaps, cs.sens
        got = []
        for r in cs.targets:
            ev = 2 * int(((ov.a_id == r) | (ov.b_id == r)).sum()) + 2 * int((sens.b_id == r).sum())
            assert cs.ds.read_len[r] <= 16384
            t = "cap 512" if ev <= 510 else "cap 1024" if ev <= 1022 else "cap 2048" if ev <= 2046 else "position space"
            assert cs.tiers[r] == t, (name, r, ev)
            got.append(t)
        if name == "cap2048":
            assert set(got) == {"cap 2048"}, got
        elif name == "position":
            assert set(got) == {"position space"}, got
        else:
            assert got.count("cap 512") >= 3 and got.count("cap 1024") >= 3 and len(got) == 8, got
            peak = [r for r in cs.targets if cs.roles[r].startswith("the peak test")]
            assert len(peak) == 1 and cs.tiers[peak[0]] in ("cap 512", "cap 1024", "cap 2048")


def test_a_floor_where_the_threshold_passes_65535_has_no_slope():
    """uint32(1.42 * v) reaches 65535 at v = 46152: no uint16 value is above it, find_slopes(1.42) flags nothing inside the
    region and there is no such hill to design.  At 46151 (threshold 65534) a plateau at 65535 still makes slopes and a hill."""
    assert int(46152 * 1.42) == 65535 and int(46151 * 1.42) == 65534
    for floor, hills in ((46152, 0), (46151, 1)):
        row = np.zeros(12000, dtype=np.uint16)
        row[15:11985] = floor
        row[4000:6000] = 65535
        o = Oracle(np.array([12000], dtype=np.uint32), None)
        o.set_pile_state(0, row, 15, 11985)
        o.find_median(0)
        inside = [(int(k) >> 1, int(l)) for k, l in o.find_slopes(0, 1.42) if 15 <= (int(k) >> 1) and int(l) < 11985]
        assert (inside != []) == bool(hills), (floor, inside)
        o.find_repetitive_hills(0, 10)
        assert len(o.intervals(0, 2)) == hills, floor


# ---- the census ----------------------------------------------------------------------------------------------------------------
def test_census_has_every_decision_on_every_side():
    seen = census()
    for d, sides in repcase.SIDES.items():
        for s in sides:
            assert (d, s) in seen, "no case takes %r on side %r" % (d, s)
    for d in repcase.PLACED:
        for s in repcase.SIDES[d]:
            assert seen[(d, s)][1] in (0, 1), "%r, side %r: the smallest margin is %d" % (d, s, seen[(d, s)][1])
    a, b = census("A"), census("B")
    for d in repcase.BY_MEDIANS:
        for s in repcase.SIDES[d]:
            assert a[(d, s)][1] in (0, 1), "%r, side %r in Layer A: the smallest margin is %d" % (d, s, a[(d, s)][1])
            assert (d, s) in b, "no Layer B case takes %r on side %r" % (d, s)


def test_census_file_is_current():
    with open(CENSUS) as f:
        assert f.read() == census_text(), "profiles/r18_repcase_census.txt is not what census_text() gives"
