"""GPU (one device): rala_hip_mg_layout_batch - the layout steps of all components of a round with the POINTS shared out over the
ranks of a sharded run (layout_shard_step_kernel per step and rank, layout_shard_fused_kernel for the components a workgroup
holds, one all-gather of the buffer just written per step).  The ranks are host threads on device 0 over the in-process
transport.  x and y equal rala_hip_layout_batch on one context as BYTES - a step is a Jacobi step, any split of the points
gives the same bits -, every rank's share is the one rala_hip_layout_split's rule gives, and `rala --gpus 2` prints the same
with RALA_LAYOUT_RANKS=1."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

import layout_batch as lb
import layout_ranks as lr

pytestmark = pytest.mark.gpu

T, DT = 0.1, 0.1 / 101
EINVAL = -2
# the mixed batch of the layout tests: the wavefront, the 256-point class and its tile, +-1 each; the fused limit +-1, a tile edge
# on a component edge (1024 = 4 tiles), a component of 6 tiles; component 3 has no adjacency; every component of at least 4
# points holds a coincident pair and a pair 1e-4 apart, partners include the origin (layout_batch.random_batch)
MIXED = (1, 6, 7, 63, 64, 65, 255, 256, 257, 300, 1023, 1024, 1025, 1300)
BATCHES = {"mixed": (MIXED, 3), "one": ((1300,), None), "fused": ((5, 64, 200, 0, 700, 1000, 256), 2),
           "holes": ((0, 9, 0, 300, 0, 70, 0), None), "small": ((9, 300, 12), None)}
_inputs, _wanted = {}, {}


def _batch(name):
    if name not in _inputs:
        sizes, bare = BATCHES[name]
        arrays = lb.random_batch(sizes, 40 + len(sizes), empty_adjacency_in=bare)
        for a in arrays:
            a.setflags(write=False)
        _inputs[name] = arrays
    return _inputs[name]


def _want(name, iterations):
    """rala_hip_layout_batch on one context: the yardstick, computed once per batch and step count"""
    if (name, iterations) not in _wanted:
        comp_off, x, y, adj_off, adj, k = _batch(name)
        ctx = hip.Context(0)
        try:
            wx, wy = x.copy(), y.copy()
            ctx.layout_batch(comp_off, wx, wy, adj_off, adj, k, iterations, T, DT)
        finally:
            ctx.close()
        wx.setflags(write=False); wy.setflags(write=False)
        _wanted[(name, iterations)] = (wx, wy)
    return _wanted[(name, iterations)]


class Group:
    """`world` ranks on device 0 that have joined one in-process group"""

    def __init__(self, world, fused_max=None):
        self.world = world
        self.group = hip.LocalGroup(world)
        self.ranks = [hip.ShardedRank(0, k, world, self.group) for k in range(world)]
        if fused_max is not None:
            for r in self.ranks:
                r.set_option("layout_fused_max", fused_max)

    def layout(self, name, iterations):
        comp_off, x, y, adj_off, adj, k = _batch(name)
        gx, gy = x.copy(), y.copy()
        hip.layout_ranks(self.ranks, comp_off, gx, gy, adj_off, adj, k, iterations, T, DT)
        return gx, gy

    def each(self, comp_off, x, y, adj_off, adj, k, iterations, download=True):
        """every rank's own call on a thread of its own: the codes, and rank 0's download"""
        gx, gy = x.copy(), y.copy()
        codes = [None] * self.world

        def one(r):
            codes[r] = self.ranks[r].layout_batch(comp_off, x, y, adj_off, adj, k, iterations, T, DT,
                                                  out=(gx, gy) if r == 0 and download else None)
        th = [threading.Thread(target=one, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return codes, gx, gy

    def close(self):
        for r in self.ranks:
            r.close()
        self.group.close()


@pytest.fixture
def group_factory():
    made = []

    def make(world, fused_max=None):
        g = Group(world, fused_max)
        made.append(g)
        return g
    yield make
    for g in made:
        g.close()


def _same_bytes(got, want):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (
        int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))


def _check_shares(g, name, fused_max, iterations):
    """every rank's info against the split computed in Python"""
    sizes = BATCHES[name][0]
    n_all = sum(sizes)
    any_tile = any(n > fused_max for n in sizes)
    infos = [r.layout_info() for r in g.ranks]
    for rank, info in enumerate(infos):
        want = lr.share(sizes, fused_max, g.world, rank)
        own = want["end_point"] - want["first_point"]
        want["launches"] = ((1 if want["components_fused_256"] else 0) + (1 if want["components_fused_1024"] else 0) +
                            (iterations if want["step_tiles"] else 0))
        want["gathers"] = iterations if any_tile else 1
        want["bytes_received"] = want["gathers"] * (n_all - own) * 16
        assert {key: info[key] for key in want} == want, (rank, info)
        assert info["device_ms"] >= 0.0 and info["exchange_ms"] >= 0.0
    return infos


@pytest.mark.parametrize("fused_max", [0, 64, 1024])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_mixed_batch_equals_one_context(group_factory, world, fused_max):
    g = group_factory(world, fused_max)
    _same_bytes(g.layout("mixed", 6), _want("mixed", 6))
    infos = _check_shares(g, "mixed", fused_max, 6)
    assert sum(i["step_tiles"] for i in infos) == sum((n + 255) // 256 for n in MIXED if n > fused_max)
    assert sum(i["components_fused_256"] + i["components_fused_1024"] for i in infos) == sum(1 for n in MIXED if n <= fused_max)


def test_one_component_cut_over_eight_ranks(group_factory):
    g = group_factory(8)
    _same_bytes(g.layout("one", 3), _want("one", 3))
    infos = _check_shares(g, "one", 1024, 3)
    idle = [i for i in infos if i["first_point"] == i["end_point"]]
    assert len(idle) == 2 and all(i["step_tiles"] == 0 and i["launches"] == 0 and i["gathers"] == 3 for i in idle)
    assert sorted(i["step_tiles"] for i in infos) == [0, 0, 1, 1, 1, 1, 1, 1]
    assert all(0 < i["end_point"] < 1300 for i in infos[:1])            # the cuts lie inside the component


@pytest.mark.parametrize("iterations", [1, 7])
def test_only_fused_components_one_gather_carries_everything(group_factory, iterations):
    g = group_factory(3)
    _same_bytes(g.layout("fused", iterations), _want("fused", iterations))
    infos = _check_shares(g, "fused", 1024, iterations)
    assert all(i["gathers"] == 1 and i["step_tiles"] == 0 for i in infos)
    assert sum(i["launches"] for i in infos) >= 2


@pytest.mark.parametrize("iterations", [1, 7])
@pytest.mark.parametrize("fused_max", [0, 256])
def test_result_buffer_parity(group_factory, iterations, fused_max):
    """odd and even step counts: the result ends up in either position buffer, with and without fused components beside tiles"""
    g = group_factory(3, fused_max)
    _same_bytes(g.layout("holes", iterations), _want("holes", iterations))
    _check_shares(g, "holes", fused_max, iterations)


def test_trivial_inputs_touch_nothing_and_exchange_nothing(group_factory):
    g = group_factory(3)
    _same_bytes(g.layout("small", 4), _want("small", 4))
    none = np.zeros(0, np.float64)
    zero_off, no_adj = np.zeros(1, np.uint32), np.zeros(0, np.uint32)
    # only empty components; no components
    hip.layout_ranks(g.ranks, np.zeros(4, np.uint32), none, none, zero_off, no_adj, np.ones(3), 50, T, DT)
    assert all(r.layout_info()["gathers"] == 0 and r.layout_info()["launches"] == 0 for r in g.ranks)
    hip.layout_ranks(g.ranks, np.zeros(0, np.uint32), none, none, np.zeros(0, np.uint32), no_adj, none, 50, T, DT)
    assert all(r.layout_info()["gathers"] == 0 and r.layout_info()["bytes_received"] == 0 for r in g.ranks)
    # no iterations: nothing moves
    x, y = _batch("small")[1], _batch("small")[2]
    _same_bytes(g.layout("small", 0), (x, y))
    assert all(r.layout_info()["gathers"] == 0 and r.layout_info()["launches"] == 0 for r in g.ranks)
    # empty components first, between and last
    _same_bytes(g.layout("holes", 2), _want("holes", 2))


def test_refused_inputs_on_every_rank_then_a_good_call(group_factory):
    g = group_factory(3)
    comp_off, x, y, adj_off, adj, k = _batch("small")
    sizes = BATCHES["small"][0]
    bad_comp = comp_off.copy()
    bad_comp[1], bad_comp[2] = comp_off[2], comp_off[1]             # decreasing, same end
    bad_start = comp_off.copy()
    bad_start[0] = 1
    bad_adj = adj.copy()
    bad_adj[0] = sizes[0] + 1                                        # the first entry belongs to component 0
    assert adj_off[sizes[0]] > 0
    bad_adj_off = adj_off.copy()
    bad_adj_off[1], bad_adj_off[2] = 7, 3
    for bad in ((bad_comp, adj_off, adj), (bad_start, adj_off, adj), (comp_off, adj_off, bad_adj), (comp_off, bad_adj_off, adj)):
        codes, gx, gy = g.each(bad[0], x, y, bad[1], bad[2], k, 4)
        assert codes == [EINVAL] * 3
        _same_bytes((gx, gy), (x, y))
        _same_bytes(g.layout("small", 4), _want("small", 4))
    # ranks that disagree on layout_fused_max would split differently: refused on every rank in the call's exchange
    g.ranks[1].set_option("layout_fused_max", 64)
    codes, gx, gy = g.each(comp_off, x, y, adj_off, adj, k, 4)
    assert codes == [EINVAL] * 3
    _same_bytes((gx, gy), (x, y))
    g.ranks[1].set_option("layout_fused_max", 1024)
    codes, gx, gy = g.each(comp_off, x, y, adj_off, adj, k, 4)
    assert codes == [0] * 3
    _same_bytes((gx, gy), _want("small", 4))


def test_calls_in_a_row_on_one_group_beside_a_run(group_factory):
    """a large call, a small one and an ordinary rala_hip_mg_run on the same rank objects: the buffers are reused, the run's
    collectives and the layout's do not disturb each other"""
    g = group_factory(3)
    ds = Dataset(600, 60_000, 9)
    cuts = hip.slice_cuts(ds.overlaps.a_id, 3, ds.overlaps.b_id)
    for rank, r in enumerate(g.ranks):
        r.set_reads(ds.read_len)
        r.set_overlaps(ds.overlaps.take(slice(cuts[rank], cuts[rank + 1])), cuts[rank])
    n_tr = hip.run_ranks(g.ranks)
    _same_bytes(g.layout("mixed", 6), _want("mixed", 6))
    _same_bytes(g.layout("small", 4), _want("small", 4))
    assert hip.run_ranks(g.ranks) == n_tr
    _same_bytes(g.layout("mixed", 6), _want("mixed", 6))
    # without a download a rank takes part all the same
    comp_off, x, y, adj_off, adj, k = _batch("small")
    codes, gx, gy = g.each(comp_off, x, y, adj_off, adj, k, 4, download=False)
    assert codes == [0] * 3
    _same_bytes((gx, gy), (x, y))


def test_cli_two_ranks_with_the_switch_print_the_same(tmp_path):
    """rala --gpus 2 on the 20x data set (tips, bubbles and long edges all occur), with and without RALA_LAYOUT_RANKS=1: the
    same contigs, debug CSV and JSON and the same four simplify counts"""
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(2000, 1_000_000, 3)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    runs = []
    for switch in (None, "1"):
        env = {key: v for key, v in os.environ.items() if key not in ("RALA_LAYOUT_RANKS", "RALA_LAYOUT_BATCH")}
        env.update(RALA_COMM="local", RALA_GPU_DEVICES="0,0")
        if switch:
            env["RALA_LAYOUT_RANKS"] = switch
        prefix = str(tmp_path / ("on" if switch else "off"))
        r = subprocess.run([exe, "-u", "-d", prefix, "--gpus", "2", fa, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=env, timeout=600)
        err = r.stderr.decode()
        assert r.returncode == 0, err[-3000:]
        counts = [l.split("] ")[1] for l in err.splitlines() if l.startswith("[rala::Graph::simplify] number of")]
        assert len(counts) == 4
        shared = re.findall(r"\[rala::Graph::postprocess\] layout by 2 ranks: (\d+) points, the largest share ([0-9.]+) % of the cost", err)
        assert (len(shared) > 0) == bool(switch), err[-3000:]
        assert all(int(p) > 0 and 50.0 <= float(s) <= 100.0 for p, s in shared)
        runs.append((r.stdout, open(prefix + ".csv").read(), open(prefix + ".json").read(), counts))
    assert runs[0][0] and runs[0] == runs[1]
    assert all(int(c.split("= ")[1]) > 0 for c in runs[0][3])
