"""The cases of tests/containcase.py do what they were designed to do, shown with the oracle alone (no device).

These are conditions on the inputs, not measurements: tests/test_gpu_containment.py can only fail for a wrong containment fixed
point if, in the oracle, every designed record deletes (or spares) its read at its stage, the chains are as deep as they claim,
and enough reads end up on either side.
"""
import numpy as np
import pytest

import containcase as cc
import parity
from oracle.oracle import Oracle


@pytest.fixture(params=sorted(cc.CASES))
def built(request):
    case = cc.case(request.param)
    return case, parity.crafted_stages(case)


def _whole_oracle(case):
    """an oracle with every read whole and annotated: the state the second pass classifies in"""
    o = Oracle(case.read_len, case.overlaps, n_threads=8)
    o.pass1()
    for r in range(case.n_reads):
        o.set_pile_state(r, cc.row_of(case, r), 0, int(case.read_len[r]))
    assert o.annotate() == 0
    return o


def _record(case, i):
    ov = case.overlaps
    return (int(ov.a_id[i]), int(ov.b_id[i]), int(ov.strand[i]),
            [int(ov.a_begin[i]), int(ov.a_end[i]), int(ov.b_begin[i]), int(ov.b_end[i]), int(ov.length[i])])


def test_the_file_is_well_formed(built):
    case, st = built
    ov = case.overlaps
    assert st["init_rc"] == 0
    a = ov.a_id.astype(np.int64)
    assert (np.diff(a) >= 0).all(), "not grouped by query"
    assert len(np.unique(a * case.n_reads + ov.b_id)) == len(ov), "a pair twice in a run"
    assert (st["valid"] == 1).all()
    assert (st["piles0"]["alive"] == 1).all() and (st["piles0"]["median"] == cc.kValue).all()
    assert (st["piles0"]["begin"] == 0).all() and (st["piles0"]["end"] == case.read_len).all()
    offs, pairs = cc.designed_pits(case)
    assert (st["pits0"][0] == offs).all() and (st["pits0"][1] == pairs).all() and len(st["hills0"][1]) == 0
    assert case.read_len.min() >= cc.kShort and case.read_len.max() <= 3600
    # the killers are listed in file order, one per record
    assert (np.diff(case.k_pos) > 0).all()


def test_designed_killers_have_their_type_at_their_stage(built):
    case, st = built
    whole = _whole_oracle(case)
    guarded = np.zeros(case.n_reads, dtype=bool)
    guarded[list(case.pit)] = True
    # pass 2: the oracle's own trim and type on whole reads; the model of Overlap::type in containcase agrees, mirrored
    for i in range(len(case.k_pos)):
        pos, stage = int(case.k_pos[i]), int(case.k_stage[i])
        a, b, strand, coords = _record(case, pos)
        ok, _, typ = whole.overlap_trim_type(a, b, strand, coords)
        mine = cc.overlap_type(int(case.read_len[a]), coords[0], coords[1], int(case.read_len[b]), coords[2], coords[3], strand)
        assert ok and typ == mine, (case.name, pos)
        target, keeper = (a, b) if typ == cc.KB else (b, a)
        if stage in (cc.PASS2, cc.TAIL0):
            assert typ == case.k_type[i] and (target, keeper) == (case.k_target[i], case.k_keeper[i]), cc.describe(case, target)
            # class 0: kept by the guard; pass 2: no guard
            assert guarded[keeper] == (stage == cc.TAIL0), cc.describe(case, target)
        else:
            assert typ == cc.KX, (case.name, pos)
    # the tail: a killer's record is in the list it is scanned from when the chimera rounds are over - unless one of its reads
    # died earlier, it is gone from both lists after the scans
    left = set(st["ov"]["src"].tolist()) | set(st["int"]["src"].tolist())
    assert not left & set(case.k_pos.tolist())
    # class 1: kB between the broken reads (the oracle with the regions of the end)
    p2 = st["piles2"]
    for i in np.nonzero(case.k_stage == cc.TAIL1)[0]:
        a, b, strand, coords = _record(case, int(case.k_pos[i]))
        assert (a, b) == (case.k_target[i], case.k_keeper[i]) and strand == 0
        for r in (a, b):
            if p2["alive"][r]:
                assert (p2["begin"][r], p2["end"][r]) == (0, cc.kBreakAt)
        la = lb = cc.kBreakAt
        assert cc.overlap_type(la, coords[0], coords[1], lb, coords[2], coords[3], 0) == cc.KB


def test_reverse_strand_coordinates_are_the_mirrored_ones():
    case = cc.case("depths")
    ov = case.overlaps
    rev = np.nonzero(ov.strand[case.k_pos] == 1)[0]
    assert len(rev) > 100 and {cc.KA, cc.KB} == set(case.k_type[rev].tolist())
    told_apart = 0
    for i in rev:
        a, b, strand, c = _record(case, int(case.k_pos[i]))
        la, lb = int(case.read_len[a]), int(case.read_len[b])
        assert cc.overlap_type(la, c[0], c[1], lb, c[2], c[3], 1) == case.k_type[i]
        told_apart += cc.overlap_type(la, c[0], c[1], lb, c[2], c[3], 1, mirror=False) != case.k_type[i]
    mirror = [c for c in case.chains if c.name.startswith("mirror_")]
    assert [c.depth for c in mirror] == [1, 2, 3] and told_apart == 6


def test_liveness_is_the_models(built):
    case, st = built
    alive = np.ones(case.n_reads, dtype=np.uint8)
    rounds = {}
    for stage, key in ((cc.PASS2, "alive_pass2"), (cc.TAIL0, None), (cc.TAIL1, "piles2")):
        died, rounds[stage] = cc.model(case, stage, st["valid"], alive)
        alive = alive & ~died
        if key is not None:
            got = st[key] if key == "alive_pass2" else st[key]["alive"]
            bad = np.nonzero(got != alive)[0]
            assert len(bad) == 0, "%s after %s: %s" % (case.name, cc.STAGE_NAMES[stage], [cc.describe(case, int(r)) for r in bad[:4]])
    # the model's rounds reach every chain's depth
    for c in case.chains:
        assert rounds[c.stage] >= c.depth, (c.name, rounds)
    # the bystanders live and their dovetails are all there
    assert alive[case.bystanders].all()
    assert len(st["edges"]["src"]) >= 4 * (len(case.bystanders) - 2) and st["n_tr"] >= len(case.bystanders) - 2


def test_both_fates_in_every_chain(built):
    case, st = built
    alive = st["piles2"]["alive"]
    for c in case.chains:
        if c.name.startswith(("descending", "ring")) or len(c.targets) < 5:
            continue
        t = np.array(c.targets)
        dead = int((alive[t] == 0).sum())
        assert 5 * dead >= len(t) and 5 * (len(t) - dead) >= len(t), (c.name, dead, len(t))
    for c in case.chains:
        t = np.array(c.targets)
        if c.name.startswith("descending"):
            assert not alive[t].any() and alive[c.reads[0]]
        if c.name.startswith("ring"):
            assert int(alive[t].sum()) == 1, c.name
            # the survivor is the member whose run is the ring's last in the file: not the first, not decided by the first record
            assert alive[max(t)] and c.reads[0] != min(t)


def test_depths_and_rounds():
    case = cc.case("depths")
    st = parity.crafted_stages(case)
    depths = {c.levels for c in case.chains}
    assert set(cc.DEPTHS) | {cc.DEEPEST} <= depths and cc.DEEPEST > 1024
    _, rounds = cc.model(case, cc.PASS2, st["valid"], np.ones(case.n_reads, dtype=np.uint8))
    assert rounds == cc.DEEPEST + 1
    names = " ".join(c.name for c in case.chains)
    assert "kB_" in names and "kA_" in names and "alt_" in names and "_reverse_" in names
    # chains are interleaved in id space and ascend along the chain
    for c in case.chains:
        assert (np.diff(c.reads) > 0).all()
    deep = [c for c in case.chains if c.levels == 300]
    assert len(deep) == 3 and max(c.reads[1] for c in deep) < min(c.reads[-1] for c in deep)
    nested = cc.case("nested_rings")
    stn = parity.crafted_stages(nested)
    for c in nested.chains:
        if c.name.startswith("nested"):
            per = c.containers
            counts = np.bincount(nested.k_target, minlength=nested.n_reads)[c.targets]
            assert counts.max() == per and (counts[7:] == per).all()
            # keepers of different fates behind one target
            a = stn["piles2"]["alive"]
            mixed = 0
            for t in c.targets[7:]:
                k = nested.k_keeper[cc.killers_of(nested, t)]
                mixed += 0 < int(a[k].sum()) < len(k)
            assert mixed > len(c.targets) // 2
            assert a[c.reads[::c.period]].all() and int(a[c.reads].sum()) == len(c.reads[::c.period])
    assert {c.levels + 1 for c in nested.chains if c.name.startswith("ring")} == set(cc.RINGS)


def test_many_at_once_is_longer_than_the_lds():
    case = cc.case("many")
    is_target = np.zeros(case.n_reads, dtype=bool)
    is_target[case.k_target] = True
    assert int(is_target[case.k_keeper].sum()) > 12288
    assert len(case.chains) == cc.MANY_CHAINS


@pytest.mark.parametrize("name", cc.TAIL_CASES)
def test_tail_cases_run_in_the_tail(name):
    case = cc.case(name)
    st = parity.crafted_stages(case)
    n2 = int((case.k_stage == cc.PASS2).sum())
    if case.name in ("guarded", "internal"):
        assert n2 == 0 and st["alive_pass2"].all()
        assert {c.depth for c in case.chains} == set(cc.TAIL_DEPTHS) == {c.levels for c in case.chains}
    kept = set(st["ov_pass2"]["src"].tolist())
    internal = set(st["int_pass2"]["src"].tolist())
    for i in range(len(case.k_pos)):
        if case.k_stage[i] == cc.TAIL0:
            assert int(case.k_pos[i]) in kept
        if case.k_stage[i] == cc.TAIL1:
            assert int(case.k_pos[i]) in internal


@pytest.mark.parametrize("flip", sorted(cc.FLIPS))
def test_crossed_records_decide(flip):
    case = cc.case("crossed")
    st = parity.crafted_stages(case)
    alive = st["piles2"]["alive"]
    assert alive[case.expect_alive].all() and not alive[case.expect_dead].any()
    # the broken guard's record is a dovetail in the end
    at = np.nonzero(st["ov"]["src"] == case.retyped)[0]
    assert len(at) == 1 and st["ov"]["type"][at[0]] == cc.KBA
    other = cc.crossed_flipped(flip)
    assert (other.read_len == case.read_len).all()
    sto = parity.crafted_stages(other)
    changed = np.nonzero(sto["piles2"]["alive"] != alive)[0].tolist()
    assert changed == other.flipped and len(changed) >= 1, (flip, [cc.describe(case, r) for r in changed])
