"""Component medians, observed bit-exactly: crafted state through rala_hip_import_state, then rala_hip_construct (needs an MI355X).

tests/compcase.py builds, per case, an overlap list whose components have designed sizes, shapes and medians, and two probe reads
per component whose pits are chimeric on either side of exactly that median; tests/test_compcase_cpu.py shows with the oracle
alone that the cases do that.  Here the state goes in through rala_hip_import_state (no piles on the device), the chimera stage
runs - cc_hook_kernel, cc_compress_count_kernel, median_fill_kernel, median_select_kernel and the spread with use_gpu_tail = 1,
the host loop around cc_hook_kernel and std::nth_element with 0 - and every read's alive / begin / end / median, both overlap
lists, the graph and the transitive marks are compared with the oracle's.
"""
import numpy as np
import pytest

from rala_amd import hip
from rala_amd.synth import Dataset

import compcase
import parity

pytestmark = pytest.mark.gpu

EINVAL, EFILTERED = -2, -4


def _import_crafted(ctx, case, st):
    offs, pairs = st["pits0"]
    aux = compcase.pit_minima(case, offs, pairs)
    ctx.set_reads(case.read_len)
    ctx.set_overlaps(case.overlaps)
    ctx.import_state(st["valid"], st["piles0"], (offs, pairs, aux), (np.zeros(case.n_reads + 1, dtype=np.uint64), np.zeros((0, 2))))


def _explain(case, st, ctx, error):
    """the case, and from the bookkeeping the component and probe of the first read whose region or liveness differs"""
    hp, op = ctx.piles(), st["piles2"]
    bad = np.nonzero((hp["alive"] != op["alive"]) | (hp["begin"] != op["begin"]) | (hp["end"] != op["end"]))[0]
    lines = ["case %s: %s" % (case.name, error)]
    for r in bad[:6].tolist():
        lines.append("  %s: [%d, %d) alive %d, the oracle has [%d, %d) alive %d" % (
            compcase.describe(case, r), hp["begin"][r], hp["end"][r], hp["alive"][r], op["begin"][r], op["end"][r], op["alive"][r]))
    if len(bad) > 6:
        lines.append("  ... and %d more reads" % (len(bad) - 6))
    return "\n".join(lines)


@pytest.mark.parametrize("gpu_tail", [1, 0])
@pytest.mark.parametrize("name", sorted(compcase.CASES))
def test_component_medians(hip_ctx_factory, name, gpu_tail):
    case = compcase.case(name)
    st = parity.crafted_stages(case)
    ctx = hip_ctx_factory()
    ctx.set_option("use_gpu_tail", gpu_tail)
    _import_crafted(ctx, case, st)
    ctx.construct()
    try:
        parity.check_construct(ctx, st)
        parity.check_tr(ctx, st)
    except AssertionError as e:
        raise AssertionError(_explain(case, st, ctx, e)) from None


@pytest.mark.parametrize("gpu_tail", [1, 0])
@pytest.mark.parametrize("n,g,seed", [(3000, 600_000, 21), (600, 60_000, 9)])
def test_round_trip_on_ordinary_data(hip_ctx_factory, n, g, seed, gpu_tail):
    """The documented use of rala_hip_import_state: what one context's initialize() found - valid bits, the per-read state, pits
    with their minima, hills - installed in a second context with the same reads and overlaps, which constructs from it."""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    first = hip_ctx_factory()
    first.set_reads(ds.read_len)
    first.set_overlaps(ds.overlaps)
    first.initialize()
    pits, hills = first.intervals(0), first.intervals(1)
    assert len(pits[1]) and len(hills[1])
    second = hip_ctx_factory()
    second.set_option("use_gpu_tail", gpu_tail)
    second.set_reads(ds.read_len)
    second.set_overlaps(ds.overlaps)
    second.import_state(first.valid(), first.piles(), pits, hills)
    assert second.num_prefiltered() == first.num_prefiltered()
    got = second.intervals(0)
    for k in range(3):
        parity.assert_same("imported pits[%d]" % k, got[k], pits[k])
    second.construct()
    parity.check_construct(second, st)
    parity.check_tr(second, st)


def test_refusals(hip_ctx_factory):
    """every refusal leaves the context usable: the good call that follows on the same context constructs as usual"""
    case = compcase.case("ties")
    st = parity.crafted_stages(case)
    offs, pairs = st["pits0"]
    aux = compcase.pit_minima(case, offs, pairs)
    none = (np.zeros(case.n_reads + 1, dtype=np.uint64), np.zeros((0, 2)), np.zeros(0))
    piles = st["piles0"]
    ctx = hip_ctx_factory()

    def good():
        ctx.import_state(st["valid"], piles, (offs, pairs, aux), none)
        parity.assert_same("alive", ctx.piles()["alive"], piles["alive"])
        assert ctx.num_prefiltered() == int((piles["alive"] == 0).sum())

    # no reads set
    with pytest.raises(hip.RalaHipError) as e:
        ctx.import_state(st["valid"], piles, (offs, pairs, aux), none)
    assert e.value.code == EINVAL
    ctx.set_reads(case.read_len)
    ctx.set_overlaps(case.overlaps)
    good()
    # overlaps set, valid bits missing (an empty array goes down as NULL)
    with pytest.raises(hip.RalaHipError) as e:
        ctx.import_state(np.zeros(0, dtype=np.uint8), piles, (offs, pairs, aux), none)
    assert e.value.code == EINVAL
    good()
    # every read dead
    dead = {k: np.zeros_like(v) for k, v in piles.items()}
    with pytest.raises(hip.RalaHipError) as e:
        ctx.import_state(st["valid"], dead, none, none)
    assert e.value.code == EFILTERED
    good()
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
