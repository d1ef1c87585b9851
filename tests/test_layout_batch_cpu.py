"""CPU: AssemblyGraph::postprocess_batched - the layouts of all components of a round through ONE engine call and one pass
over the edges (reference graph.cpp:1056-1279 does a component at a time) - against the oracle's postprocess and the
product's own per-component postprocess, exactly (== on float64).  The engine is the numpy yardstick (layout.numpy_engine
per component), never the code under test."""
import numpy as np
import pytest

import layout
import layout_batch as lb
import test_layout_cpu as cpu


def _graphs(seed, n=2):
    graphs = tuple([layout.product() for _ in range(n - 1)] + [layout.oracle()])
    n_tangles = lb.multi_tangle(graphs, seed)
    return graphs, n_tangles


@pytest.mark.parametrize("seed", range(12))
def test_batched_matches_oracle_and_per_component(seed):
    (batched, single, ora), n_tangles = _graphs(seed, 3)
    calls = []

    def engine(comp_off, *rest):
        calls.append(len(comp_off) - 1)
        return lb.numpy_batch_engine(comp_off, *rest)

    lb.Batched(batched).postprocess(seed, engine)
    single.postprocess(seed)
    ora.postprocess(seed)
    assert calls == [n_tangles]                   # one call; the chain and the small component are skipped
    layout.assert_same_graph(batched, ora, "batched against the oracle")
    layout.assert_same_graph(batched, single, "batched against per-component")
    assert (batched.edge_weights() > 0).any()


@pytest.mark.parametrize("seed", [0, 1, 4, 7])
def test_batch_slices_are_the_per_component_arguments(seed):
    (batched, single, _), n_tangles = _graphs(seed, 3)
    one_by_one, sliced = [], []

    def engine(x, y, adj_off, adj, iterations, k, t, dt):
        one_by_one.append((x.copy(), y.copy(), adj_off.copy(), adj.copy(), iterations, k, t, dt))
        return layout.numpy_engine(x, y, adj_off, adj, iterations, k, t, dt)

    def batch_engine(comp_off, x, y, adj_off, adj, k, iterations, t, dt):
        for cx, cy, off, a, kc in lb.component_slices(comp_off, x, y, adj_off, adj, k):
            sliced.append((cx.copy(), cy.copy(), off, a, iterations, kc, t, dt))
        return lb.numpy_batch_engine(comp_off, x, y, adj_off, adj, k, iterations, t, dt)

    single.postprocess(seed, engine)
    lb.Batched(batched).postprocess(seed, batch_engine)
    assert len(one_by_one) == len(sliced) == n_tangles
    crossing = False
    for a, b in zip(one_by_one, sliced):
        for u, v in zip(a[:4], b[:4]):
            assert u.dtype == v.dtype and u.shape == v.shape and (u == v).all()
        assert a[4:] == b[4:]
        crossing = crossing or (len(a[3]) and int(a[3].max()) == len(a[0]))
    assert crossing                               # the bridge's partner sits at the origin of its component
    layout.assert_same_graph(batched, single, "after both")


@pytest.mark.parametrize("seed", range(12))
def test_simplify_through_the_batched_entry(seed):
    (prod, ora), _ = _graphs(seed)
    la, lo = [], []
    cpu._simplify(lb.Batched(prod), la)
    cpu._simplify(ora, lo)
    assert la == lo                               # tips, bubbles, long edges per round
    layout.assert_same_graph(prod, ora, "after simplify")
