"""Helpers of the tests of the batched layout (AssemblyGraph::postprocess_batched, rala_hip_layout_batch): the ctypes binding
of ag_postprocess_batched, the numpy yardstick (layout.numpy_engine component by component), a graph of several tangles, and
random layout inputs without a graph."""
import ctypes

import numpy as np

import layout

_D, _U = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
BATCH_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint32, _U, _D, _D, _U, _U, _D, ctypes.c_uint32, ctypes.c_double,
                            ctypes.c_double)


def component_slices(comp_off, x, y, adj_off, adj, k):
    """the arguments of a per-component engine for every component of a batch: (x, y, adj_off, adj, k) with x / y views"""
    for c in range(len(comp_off) - 1):
        lo, hi = int(comp_off[c]), int(comp_off[c + 1])
        a_lo, a_hi = (int(adj_off[lo]), int(adj_off[hi])) if len(adj_off) else (0, 0)
        yield (x[lo:hi], y[lo:hi], (adj_off[lo:hi + 1] - adj_off[lo]).astype(np.uint32), adj[a_lo:a_hi].copy(), float(k[c]))


def numpy_batch_engine(comp_off, x, y, adj_off, adj, k, iterations, t, dt):
    """the yardstick: layout.numpy_engine on every component's slice in turn"""
    for cx, cy, off, a, kc in component_slices(comp_off, x, y, adj_off, adj, k):
        if len(cx):
            layout.numpy_engine(cx, cy, off, a, iterations, kc, t, dt)
    return 0


def per_component(engine):
    """a batch engine out of a per-component one (engine(x, y, adj_off, adj, iterations, k, t, dt))"""
    def batch(comp_off, x, y, adj_off, adj, k, iterations, t, dt):
        for cx, cy, off, a, kc in component_slices(comp_off, x, y, adj_off, adj, k):
            if len(cx):
                gx, gy = cx.copy(), cy.copy()
                engine(gx, gy, off, a, iterations, kc, t, dt)
                cx[:] = gx; cy[:] = gy
        return 0
    return batch


def batch_callback(fn):
    """wraps engine(comp_off, x, y, adj_off, adj, k, iterations, t, dt) (numpy arrays, x / y in place)"""
    def raw(n_components, pcomp, px, py, poff, padj, pk, iterations, t, dt):
        comp_off = np.ctypeslib.as_array(pcomp, shape=(n_components + 1,)).copy()
        n = int(comp_off[-1])
        x = np.ctypeslib.as_array(px, shape=(n,)); y = np.ctypeslib.as_array(py, shape=(n,))
        off = np.ctypeslib.as_array(poff, shape=(n + 1,)).copy()
        adj = np.ctypeslib.as_array(padj, shape=(int(off[n]),)).copy() if off[n] else np.zeros(0, np.uint32)
        k = np.ctypeslib.as_array(pk, shape=(n_components,)).copy()
        return int(fn(comp_off, x, y, off, adj, k, iterations, t, dt))
    return BATCH_FN(raw)


class Batched:
    """a product graph whose postprocess goes through ag_postprocess_batched; everything else is the graph's own"""

    def __init__(self, gph):
        self.g = gph
        fn = gph.L.ag_postprocess_batched
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, BATCH_FN]
        fn.restype = ctypes.c_int
        self.fn = fn

    def postprocess(self, seed, engine=None):
        cb = batch_callback(engine or numpy_batch_engine)
        assert self.fn(self.g.h, seed, cb) == 0

    def __getattr__(self, name):
        return getattr(self.g, name)


def multi_tangle(graphs, seed):
    """1 to 5 tangles of different sizes on disjoint read ids (each as test_layout_cpu._tangle builds one: chains that cross in
    shared nodes, shortcuts marked as transitive and removed), a plain chain without a junction (at least 6 nodes: skipped for
    want of a junction), a component of 4 nodes (skipped for its size), and one bridge edge between two components - the first
    two tangles, or the only tangle and the chain - that is marked transitive and removed too, so a remembered transitive pair
    crosses two components.  Returns the number of tangles."""
    rng = np.random.default_rng(1000 + seed)
    n_tangles = 1 + seed % 5
    edges, marked, first_of = [], [], []
    n_reads = 0
    for i in range(n_tangles):
        n_chains, length = int(rng.integers(2, 4)), 8 + 3 * i + int(rng.integers(0, 3))
        ids = [[n_reads + c * length + k for k in range(length)] for c in range(n_chains)]
        first_of.append(n_reads)
        n_reads += n_chains * length
        for ch in ids:
            for a, b in zip(ch, ch[1:]):
                edges.append((a, b, int(rng.integers(1000, 3000))))
        for c in range(1, n_chains):                       # cross links through the middle
            edges.append((ids[0][length // 2], ids[c][length // 2 + 1], 2500))
            edges.append((ids[c][length // 2 - 1], ids[0][length // 2], 2500))
        for _ in range(4):
            c = int(rng.integers(0, n_chains)); k = int(rng.integers(0, length - 3))
            marked.append(len(edges))
            edges.append((ids[c][k], ids[c][k + 2], 5000))
    chain = list(range(n_reads, n_reads + 8))
    n_reads += 8
    for a, b in zip(chain, chain[1:]):
        edges.append((a, b, 2000))
    small = list(range(n_reads, n_reads + 4))              # a junction, but four nodes only
    n_reads += 4
    edges += [(small[0], small[1], 2000), (small[0], small[2], 2100), (small[1], small[3], 2000)]
    marked.append(len(edges))
    edges.append((first_of[0] + 1, first_of[1] + 2 if n_tangles > 1 else chain[3], 5000))
    for gph in graphs:
        r = np.random.default_rng(seed)
        for k in range(n_reads):
            gph.add_node_pair(k, b"r%d" % k, bytes(r.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=9000)))
        for a, b, l in edges:
            gph.add_edge(2 * a, 2 * b, l)
            gph.add_edge(2 * b + 1, 2 * a + 1, l)
        for e in marked:
            gph.mark_edge(2 * e)
        gph.note_transitive()
        gph.remove_marked(False)
    return n_tangles


def random_batch(sizes, seed, empty_adjacency_in=None):
    """layout inputs without a graph: per component random points, in every component of at least 4 points a coincident pair
    and a pair 1e-4 apart (the 0.01 clamps), degrees 0-5, partners that include the origin index n_c, k = sqrt(1 / n_c);
    component `empty_adjacency_in` has no adjacency at all.  Returns comp_off, x, y, adj_off, adj, k."""
    rng = np.random.default_rng(seed)
    comp_off = np.zeros(len(sizes) + 1, dtype=np.uint32)
    np.cumsum(np.asarray(sizes, dtype=np.uint32), out=comp_off[1:])
    n_all = int(comp_off[-1])
    x, y = rng.random(n_all), rng.random(n_all)
    deg = np.zeros(n_all, dtype=np.int64)
    adj = []
    for c, n in enumerate(sizes):
        lo = int(comp_off[c])
        if n >= 4:
            x[lo + 1], y[lo + 1] = x[lo], y[lo]
            x[lo + 2], y[lo + 2] = x[lo] + 1e-4, y[lo]
        if n == 0 or c == empty_adjacency_in:
            continue
        d = rng.integers(0, 6, size=n)
        if n >= 6:
            d[:6] = np.arange(6)                           # every degree 0-5 occurs
        deg[lo:lo + n] = d
        a = rng.integers(0, n + 1, size=int(d.sum())).astype(np.uint32)
        if len(a):
            a[-1] = n                                      # the origin
        adj.append(a)
    adj_off = np.zeros(n_all + 1, dtype=np.uint32)
    np.cumsum(deg, out=adj_off[1:])
    adj = np.concatenate(adj).astype(np.uint32) if adj else np.zeros(0, np.uint32)
    k = np.array([np.sqrt(1.0 / n) if n else 1.0 for n in sizes], dtype=np.float64)
    return comp_off, x, y, adj_off, adj, k
