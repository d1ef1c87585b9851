"""Containment removal on crafted chains, rings and nested reads: state through rala_hip_import_state, then rala_hip_construct
(needs an MI355X).

tests/containcase.py builds overlap lists whose in-order containment removal is up to 1 100 levels deep - in the second pass, in
the tail's scan over the overlaps and in the one over the internals - with several killers per target, keeper cycles, and scans
whose outcome depends on the other scan's; tests/test_containcase_cpu.py shows with the oracle alone that the cases do that.  Here
the device solves them as fixed points (death_decide rounds, fixed_point_kernels.hip in LDS and across workgroups, the host's
loop of one look per round, tail_contain_collect / _reduce) and everything construct leaves - every read's alive / begin / end /
median, both overlap lists, the graph, the transitive marks - is compared with the oracle's.

Crossings that are left out because they reach no other code: the fixed-point options only reach the tail's scans when the tail
runs on the device, and use_round_batches only the second pass.  So the tail cases run use_gpu_tail = 0 once, with no option, and
`guarded` and `internal`, which have no killer in the second pass at all, do not run use_round_batches = 0.
"""
import numpy as np
import pytest

from rala_amd.synth import Dataset

import containcase as cc
import parity

pytestmark = pytest.mark.gpu

OPTION_SETS = [{}, {"debug_fp_lds_limit": 0}, {"debug_fp_lds_limit": 40}, {"use_round_batches": 0},
               {"debug_fp_lds_limit": 0, "debug_fp_give_up": 1}, {"debug_fp_lds_limit": 0, "debug_fp_give_up": 2}]


def _crossings():
    out = []
    for name in cc.PASS2_CASES:
        out += [(name, opts, tail) for opts in OPTION_SETS for tail in (1, 0)]
    for name in cc.TAIL_CASES:
        for opts in OPTION_SETS:
            if "use_round_batches" in opts and name != "crossed":
                continue
            out.append((name, opts, 1))
        out.append((name, {}, 0))
    return out


def _id(v):
    if isinstance(v, dict):
        return "-".join("%s=%d" % (k.replace("debug_fp_", "").replace("use_", ""), x) for k, x in v.items()) or "default"
    return str(v)


def _import_crafted(ctx, case, st):
    offs, pairs = st["pits0"]
    aux = cc.pit_minima(case, offs, pairs)
    ctx.set_reads(case.read_len)
    ctx.set_overlaps(case.overlaps)
    ctx.import_state(st["valid"], st["piles0"], (offs, pairs, aux), (np.zeros(case.n_reads + 1, dtype=np.uint64), np.zeros((0, 2))))


def _explain(case, st, ctx, error):
    """the case, and from the bookkeeping the first reads whose liveness or region differs"""
    hp, op = ctx.piles(), st["piles2"]
    bad = np.nonzero((hp["alive"] != op["alive"]) | (hp["begin"] != op["begin"]) | (hp["end"] != op["end"]))[0]
    lines = ["case %s: %s" % (case.name, error), "  %d reads differ" % len(bad)]
    for r in bad[:6].tolist():
        lines.append("  %s: [%d, %d) alive %d, the oracle has [%d, %d) alive %d (alive after its second pass: %d)" % (
            cc.describe(case, r), hp["begin"][r], hp["end"][r], hp["alive"][r], op["begin"][r], op["end"][r], op["alive"][r],
            st["alive_pass2"][r]))
    if len(bad) > 6:
        lines.append("  ... and %d more reads" % (len(bad) - 6))
    return "\n".join(lines)


def _construct_and_check(ctx, case, st):
    _import_crafted(ctx, case, st)
    ctx.construct()
    try:
        parity.check_construct(ctx, st)
        parity.check_tr(ctx, st)
    except AssertionError as e:
        raise AssertionError(_explain(case, st, ctx, e)) from None


@pytest.mark.parametrize("name,opts,gpu_tail", _crossings(), ids=_id)
def test_containment(hip_ctx_factory, name, opts, gpu_tail):
    case = cc.case(name)
    st = parity.crafted_stages(case)
    ctx = hip_ctx_factory()
    ctx.set_option("use_gpu_tail", gpu_tail)
    for k, v in opts.items():
        ctx.set_option(k, v)
    _construct_and_check(ctx, case, st)
    rounds = ctx.timings()["death_rounds"]
    deepest = max(c.depth for c in case.chains if c.stage == cc.PASS2) if name in cc.PASS2_CASES else 0
    print("%s: %d reads, %d designed killers, deepest pass-2 chain %d, death_rounds %d" % (
        name, case.n_reads, len(case.k_pos), deepest, rounds))
    # the iteration is antitone and yields an upper and a lower bound in turn: no correct solver settles more than two levels
    # of a chain per round - the floor only shows that the deep path ran
    assert rounds >= deepest // 2, (rounds, deepest)


@pytest.mark.parametrize("opts", [{}, {"debug_fp_lds_limit": 40}, {"debug_fp_lds_limit": 0, "debug_fp_give_up": 2}], ids=_id)
def test_one_context_after_another_case(hip_ctx_factory, opts):
    """two different cases, then an ordinary data set, on ONE context: the maps, counters and work arrays that the fixed points
    leave all ones (or zero) between calls are really left that way, after a thousand rounds too"""
    ctx = hip_ctx_factory()
    for k, v in opts.items():
        ctx.set_option(k, v)
    for name in ("nested_rings", "depths", "internal"):
        case = cc.case(name)
        _construct_and_check(ctx, case, parity.crafted_stages(case))
    ds = Dataset(3000, 600_000, 21)
    st = parity.oracle_stages(ds)
    parity.run_hip(ctx, ds)
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    # ... and a crafted case again behind the ordinary one
    case = cc.case("crossed")
    _construct_and_check(ctx, case, parity.crafted_stages(case))
