"""GPU: rala_hip_layout_batch - the force-directed layout steps of all components of a round in one call (reference
graph.cpp:1132-1226 per component): components a workgroup holds run fused in one launch (layout_fused_kernel), larger
ones step by step together (layout_batch_step_kernel).  Bit-identical (== on float64) to layout.numpy_engine per component
and to rala_hip_layout per component, on every path; alone, inside the clean-up pipeline against the oracle, and in `rala`."""
import os
import subprocess

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

import layout
import layout_batch as lb
import test_layout_cpu as cpu

pytestmark = pytest.mark.gpu

T, DT = 0.1, 0.1 / 101
# (sizes, iterations, component without adjacency): the wavefront, the 256-point class and its tile, +-1 each, with the
# reference's 50 steps; then the fused limit +-1, a tile edge on a component edge (1024 = 4 tiles) and a small component behind
# large ones, with 6 steps (the numpy yardstick is O(n^2) per step in Python)
CALLS = {"small": ((1, 6, 7, 63, 64, 65, 255, 256, 257), 50, 3), "large": ((300, 1023, 1024, 1025, 1300, 6), 6, 0)}
_cache = {}


def _call(name):
    """the inputs of a call and what numpy_engine makes of every component, computed once"""
    if name not in _cache:
        sizes, iterations, bare = CALLS[name]
        inputs = lb.random_batch(sizes, 11 + len(sizes), empty_adjacency_in=bare)
        comp_off, x, y, adj_off, adj, k = inputs
        wx, wy = x.copy(), y.copy()
        lb.numpy_batch_engine(comp_off, wx, wy, adj_off, adj, k, iterations, T, DT)
        for a in inputs + (wx, wy):
            a.setflags(write=False)
        _cache[name] = (inputs, iterations, wx, wy)
    return _cache[name]


def _expected_info(sizes, fused_max, iterations):
    """which path a component takes by the documented rule (not by asking the library)"""
    c256 = [n for n in sizes if 0 < n <= min(fused_max, 256)]
    c1024 = [n for n in sizes if 256 < n <= fused_max]
    stepped = [n for n in sizes if n > fused_max]
    tiles = sum((n + 255) // 256 for n in stepped)
    return {"components_fused_256": len(c256), "components_fused_1024": len(c1024), "components_stepped": len(stepped),
            "components_empty": sum(1 for n in sizes if n == 0), "points_fused_256": sum(c256), "points_fused_1024": sum(c1024),
            "points_stepped": sum(stepped), "step_tiles": tiles,
            "launches": (iterations if stepped else 0) + (1 if c256 else 0) + (1 if c1024 else 0) if iterations else 0}


def _check_info(ctx, sizes, fused_max, iterations):
    info = ctx.layout_info()
    want = _expected_info(sizes, fused_max, iterations)
    assert {key: info[key] for key in want} == want
    assert info["device_ms"] >= 0.0
    return info


def _batch(ctx, inputs, iterations):
    comp_off, x, y, adj_off, adj, k = inputs
    gx, gy = x.copy(), y.copy()
    ctx.layout_batch(comp_off, gx, gy, adj_off, adj, k, iterations, T, DT)
    return gx, gy


@pytest.mark.parametrize("fused_max", [0, 64, 1024])
@pytest.mark.parametrize("name", ["small", "large"])
def test_mixed_sizes_on_every_path(hip_ctx_factory, name, fused_max):
    inputs, iterations, wx, wy = _call(name)
    ctx = hip_ctx_factory()
    ctx.set_option("layout_fused_max", fused_max)
    gx, gy = _batch(ctx, inputs, iterations)
    info = _check_info(ctx, CALLS[name][0], fused_max, iterations)
    if fused_max == 1024:
        assert info["components_fused_256"] > 0 and info["points_fused_256"] > 0
        assert name == "small" or (info["components_fused_1024"] == 3 and info["components_stepped"] == 2)
    assert (gx == wx).all() and (gy == wy).all(), (np.abs(gx - wx).max(), np.abs(gy - wy).max())
    # ... and rala_hip_layout on every component's slice in turn
    comp_off, x, y, adj_off, adj, k = inputs
    sx, sy = x.copy(), y.copy()
    lb.per_component(ctx.layout)(comp_off, sx, sy, adj_off, adj, k, iterations, T, DT)
    assert (gx == sx).all() and (gy == sy).all()


def test_valid_trivial_inputs(hip_ctx_factory):
    ctx = hip_ctx_factory()
    none = np.zeros(0, np.float64)
    ctx.layout_batch(np.zeros(1, np.uint32), none, none, np.zeros(1, np.uint32), np.zeros(0, np.uint32), none, 50, T, DT)
    ctx.layout_batch(np.zeros(0, np.uint32), none, none, np.zeros(0, np.uint32), np.zeros(0, np.uint32), none, 50, T, DT)
    assert ctx.layout_info()["launches"] == 0
    # an empty component first, in the middle and last
    sizes = (0, 9, 0, 70, 0)
    inputs = lb.random_batch(sizes, 5)
    comp_off, x, y, adj_off, adj, k = inputs
    wx, wy = x.copy(), y.copy()
    lb.numpy_batch_engine(comp_off, wx, wy, adj_off, adj, k, 7, T, DT)
    gx, gy = _batch(ctx, inputs, 7)
    assert _check_info(ctx, sizes, 1024, 7)["components_empty"] == 3
    assert (gx == wx).all() and (gy == wy).all()
    # only empty components
    ctx.layout_batch(np.zeros(4, np.uint32), none, none, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.ones(3), 50, T, DT)
    assert ctx.layout_info()["components_empty"] == 3 and ctx.layout_info()["launches"] == 0
    # no iterations: nothing moves
    gx, gy = _batch(ctx, inputs, 0)
    assert (gx == x).all() and (gy == y).all() and ctx.layout_info()["launches"] == 0


def test_refused_inputs_touch_nothing(hip_ctx_factory):
    ctx = hip_ctx_factory()
    sizes = (9, 300, 12)
    inputs = lb.random_batch(sizes, 6)
    comp_off, x, y, adj_off, adj, k = inputs
    wx, wy = x.copy(), y.copy()
    lb.numpy_batch_engine(comp_off, wx, wy, adj_off, adj, k, 5, T, DT)

    def good_call():
        gx, gy = _batch(ctx, inputs, 5)
        assert (gx == wx).all() and (gy == wy).all()

    def refused(fn):
        with pytest.raises(hip.RalaHipError) as e:
            fn()
        assert e.value.code == -2                  # RALA_HIP_EINVAL

    bad_comp = comp_off.copy()
    bad_comp[1], bad_comp[2] = comp_off[2], comp_off[1]           # decreasing, same end
    bad_adj = adj.copy()
    bad_adj[0] = sizes[0] + 1                                      # the first entry belongs to component 0
    assert adj_off[sizes[0]] > 0
    for bad in ((bad_comp, adj), (comp_off, bad_adj)):
        gx, gy = x.copy(), y.copy()
        refused(lambda: ctx.layout_batch(bad[0], gx, gy, adj_off, bad[1], k, 5, T, DT))
        assert (gx == x).all() and (gy == y).all()
        good_call()
    refused(lambda: ctx.set_option("layout_fused_max", 1025))
    good_call()
    _check_info(ctx, sizes, 1024, 5)               # the refused value did not replace the default


def test_buffers_are_reused_across_calls(hip_ctx_factory):
    ctx = hip_ctx_factory()
    inputs, iterations, wx, wy = _call("large")
    gx, gy = _batch(ctx, inputs, iterations)
    assert (gx == wx).all() and (gy == wy).all()
    inputs, iterations, wx, wy = _call("small")
    gx, gy = _batch(ctx, inputs, iterations)
    assert (gx == wx).all() and (gy == wy).all()
    comp_off, x, y, adj_off, adj, k = inputs                       # then rala_hip_layout on one component (257 points)
    lo, hi = int(comp_off[-2]), int(comp_off[-1])
    sx, sy = x[lo:hi].copy(), y[lo:hi].copy()
    ctx.layout(sx, sy, adj_off[lo:hi + 1] - adj_off[lo], adj[int(adj_off[lo]):int(adj_off[hi])], iterations, float(k[-1]), T, DT)
    assert (sx == wx[lo:hi]).all() and (sy == wy[lo:hi]).all()


def _device_engine(ctx, seen):
    def engine(comp_off, x, y, adj_off, adj, k, iterations, t, dt):
        ctx.layout_batch(comp_off, x, y, adj_off, adj, k, iterations, t, dt)
        seen.append(ctx.layout_info())
        return 0
    return engine


@pytest.mark.parametrize("seed", range(5))
def test_layout_batch_in_the_pipeline(hip_ctx_factory, seed):
    ctx = hip_ctx_factory()
    graphs = cpu._both()
    n_tangles = lb.multi_tangle(graphs, seed)
    prod, ora = lb.Batched(graphs[0]), graphs[1]
    seen = []
    prod.postprocess(seed, _device_engine(ctx, seen))
    ora.postprocess(seed)
    assert len(seen) == 1 and seen[0]["components_fused_256"] == n_tangles and seen[0]["launches"] == 1
    layout.assert_same_graph(graphs[0], ora, "after postprocess")
    assert (graphs[0].edge_weights() > 0).any()
    la, lo = [], []
    cpu._simplify(prod, la, _device_engine(ctx, seen))
    cpu._simplify(ora, lo)
    assert la == lo
    layout.assert_same_graph(graphs[0], ora, "after simplify")


def test_cli_with_the_switch_prints_the_same(tmp_path):
    """RALA_LAYOUT_BATCH=1 rala on the 20x data set (tips, bubbles and long edges all occur): the same contigs and counts"""
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(2000, 1_000_000, 3)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    runs = []
    for switch in (None, "1"):
        env = {key: v for key, v in os.environ.items() if key != "RALA_LAYOUT_BATCH"}
        if switch:
            env["RALA_LAYOUT_BATCH"] = switch
        r = subprocess.run([exe, "-u", fa, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0, r.stderr.decode()
        counts = [l.split("] ")[1] for l in r.stderr.decode().splitlines()
                  if l.startswith("[rala::Graph::simplify] number of")]
        assert len(counts) == 4 and "[rala::Graph::postprocess]" in r.stderr.decode()
        runs.append((r.stdout, counts))
    assert runs[0][0] and runs[0] == runs[1]
    assert all(int(c.split("= ")[1]) > 0 for c in runs[0][1])
