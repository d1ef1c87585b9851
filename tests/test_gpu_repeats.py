"""The sensitive pass on designed repeat hills, branch by branch (needs an MI355X).

tests/repcase.py designs the cases and holds a plain model that names every decision of Pile::find_repetitive_hills,
check_repetitive_hills and is_valid_overlap; tests/test_repcase_cpu.py shows with the oracle alone that the cases sit on the
compares they were aimed at.  Here Layer A goes through rala_hip_find_repetitive_hills, one read per call (the position-space
kernel: lists in LDS, lists in global memory that double, rows in HBM slabs), and Layer B through rala_hip_initialize and
rala_hip_construct with the sensitive set: the designed targets of the three sets start in the cap-512 and cap-1024, the
cap-2048 and the position-space kernel of mode 2 (test_repcase_cpu.py::test_tiers); the bridge and the filter run on the device
and in the host tail.  A failing comparison prints the model's trace of the first
read that differs: which decision, which side, what margin.
"""
import numpy as np
import pytest

from rala_amd import hip

import parity
import repcase
from test_gpu_sharded import sharded_factory  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


# ---- Layer A -------------------------------------------------------------------------------------------------------------------
def _hills_of(iv, r):
    offs, pairs, flags = iv
    lo, hi = int(offs[r]), int(offs[r + 1])
    return [tuple(int(v) for v in x) for x in pairs[lo:hi]], [int(f) for f in flags[lo:hi]]


@pytest.mark.parametrize("options", [{}, {"debug_force_big": 1, "debug_big_caps": (4 << 32) | 4}, {"max_lds_read_len": 0}],
                         ids=["default", "lists_that_double", "slab"])
def test_stand_alone_entry(hip_ctx_factory, options):
    """per call of rala_hip_find_repetitive_hills the read's intervals of kind 2 are the oracle's (the model's, which
    test_repcase_cpu.py shows to be the oracle's), flags all zero; every earlier read's hills are still reported"""
    A = repcase.layer_a()
    ctx = hip_ctx_factory()
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_reads(A.read_len)
    ctx.set_overlaps(A.overlaps)
    ctx.initialize()
    for c in A.calls:
        assert (ctx.pile_data(c.read) == c.row).all(), c.name
    unbounded = ctx.timings()["pile_unbounded_reads"]
    for k, c in enumerate(A.calls):
        ctx.find_repetitive_hills(c.read, c.begin, c.end, c.median, c.p10, c.dm)
        iv = ctx.intervals(2)
        hills, flags = _hills_of(iv, c.read)
        assert hills == c.hills and not any(flags), "%s: the device has %s flags %s, the oracle %s\n%s" % (
            c.name, hills, flags, c.hills, "\n".join("    %-48s %-8s margin %d" % d for d in c.log))
        if k == 1:
            first = A.calls[0]
            assert _hills_of(iv, first.read)[0] == first.hills and first.hills, "the first read's hills are gone after the second call"
    iv = ctx.intervals(2)
    for c in A.calls:
        assert _hills_of(iv, c.read) == (c.hills, [0] * len(c.hills)), c.name
    assert iv[0][-1] == sum(len(c.hills) for c in A.calls)
    if "debug_force_big" in options:
        assert ctx.timings()["pile_unbounded_reads"] > unbounded


# ---- Layer B -------------------------------------------------------------------------------------------------------------------
def _explain(cs, ctx, error):
    """the model's trace of the first read whose hills or flags differ, or of the two reads of the first overlap that does"""
    lines = ["case set %s: %s" % (cs.name, error)]
    st = cs.st
    got, want = ctx.intervals(2), (st["rep"][0], st["rep"][1], st["flags"])
    for r in range(cs.ds.n_reads):
        if _hills_of(got, r) != _hills_of(want, r):
            lines.append("read %d%s: the device has %s" % (r, " (%s)" % cs.roles[r] if r in cs.roles else "", _hills_of(got, r)))
            lines.append(cs.trace.describe(r))
            return "\n".join(lines)
    h = set(ctx.overlap_list(0)["src"].tolist())
    o = set(st["ov"]["src"].tolist())
    front = st["front"].ov
    for k in sorted(h ^ o)[:1]:
        i = np.nonzero(front["src"] == k)[0]
        lines.append("overlap %d: kept by the device %s, by the oracle %s" % (k, k in h, k in o))
        for r in ([int(front["a_id"][i[0]]), int(front["b_id"][i[0]])] if len(i) else []):
            lines.append(cs.trace.describe(r))
    return "\n".join(lines)


def _compare(cs, ctx, pile_data=None):
    """what _check_sensitive of tests/test_gpu_parity.py compares, and the rows of every designed target"""
    st = cs.st
    try:
        offs, pairs, flags = ctx.intervals(2)
        parity.assert_same("rep.offsets", offs, st["rep"][0])
        parity.assert_same("rep.pairs", pairs, st["rep"][1])
        parity.assert_same("rep.flags", flags.astype(np.uint8), st["flags"])
        hp = ctx.piles()
        for k in ("alive", "begin", "end", "median", "p10"):
            parity.assert_same("piles." + k, hp[k], st["piles"][k])
        parity.assert_same("ov.src", ctx.overlap_list(0)["src"], st["ov"]["src"].astype(np.uint32))
    except AssertionError as e:
        raise AssertionError(_explain(cs, ctx, e)) from None
    for r in cs.targets:
        parity.assert_same("pile_data[%d]" % r, (pile_data or ctx.pile_data)(r), st["data"][r])


def _graph(cs, ctx, n_tr):
    assert n_tr == cs.st["n_tr"]
    gr = ctx.graph()
    for k in ("src", "dst", "len", "marked"):
        parity.assert_same("edges." + k, gr[k], cs.st["edges"][k])


VARIANTS = {
    "default": {},
    "position_space": {"use_run_kernel": 0},
    "host_tail": {"use_gpu_tail": 0},
    "lists_that_double": {"use_run_kernel": 0, "debug_force_big": 1, "debug_big_caps": (4 << 32) | 4},
    "no_resident_rows": {"pile_rows": 0},
    "no_side_stream": {"use_side_stream": 0},
    "sensitive_in_device_memory": {"sensitive_in_device_memory": 1},
    "pools_that_grow": {"interval_pool_per_read_x1000": 0},
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(repcase.BASES))
def test_construct_with_designed_records(hip_ctx_factory, name, variant):
    cs = repcase.case_set(name)
    ctx = hip_ctx_factory()
    for k, v in VARIANTS[variant].items():
        if k != "sensitive_in_device_memory":
            ctx.set_option(k, v)
    ctx.set_reads(cs.ds.read_len)
    ctx.set_overlaps(cs.ds.overlaps)
    ctx.initialize()
    if variant == "sensitive_in_device_memory":
        ctx.set_option("sensitive_in_device_memory", 1)
        ctx.construct(hip.DeviceOverlaps.from_host(cs.sens, 0))
    else:
        ctx.construct(cs.sens)
    if variant == "pools_that_grow" and len(cs.st["rep"][1]) > 16:          # (both pools start at 16 slots)
        assert ctx.timings()["pool_regrown"] >= 1, ctx.timings()
    _compare(cs, ctx)
    _graph(cs, ctx, ctx.remove_transitive_edges())


@pytest.mark.parametrize("name", sorted(repcase.BASES))
def test_construct_twice_on_one_context(hip_ctx_factory, name):
    """a second initialize and construct with the same device-resident set: it is not consumed, nothing is left over"""
    cs = repcase.case_set(name)
    ctx = hip_ctx_factory()
    ctx.set_reads(cs.ds.read_len)
    ctx.set_overlaps(cs.ds.overlaps)
    ctx.initialize()
    ctx.set_option("sensitive_in_device_memory", 1)
    dev = hip.DeviceOverlaps.from_host(cs.sens, 0)
    ctx.construct(dev)
    _compare(cs, ctx)
    ctx.initialize()
    ctx.construct(dev)
    _compare(cs, ctx)
    _graph(cs, ctx, ctx.remove_transitive_edges())


def test_three_ranks(sharded_factory):
    cs = repcase.case_set("cap2048")
    world = 3
    sh = sharded_factory(cs.ds, world)
    n_tr = sh.run(cs.sens)
    for rank in sh.ranks:
        ctx = rank.context()
        _compare(cs, ctx, pile_data=lambda r: sh.ranks[r % world].pile_data(r))
        _graph(cs, ctx, n_tr)
