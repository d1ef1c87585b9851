"""Stage-by-stage comparison of the HIP path (through the C ABI) with the oracle."""
import numpy as np

from oracle.oracle import Oracle


def oracle_stages(ds, n_threads=8, ref=False, with_tr=True, n_data=64, data_of=()):
    """Run the oracle on a synthetic data set, snapshotting every stage."""
    o = Oracle(ds.read_len, ds.overlaps, n_threads=n_threads, ref=ref)
    st = {}
    rc = o.initialize()
    st["init_rc"] = rc
    st["valid"] = o.valid()
    st["piles0"] = o.piles()
    st["pits0"] = o.all_intervals(0)
    st["hills0"] = o.all_intervals(1)
    st["oracle"] = o
    st["rows0"] = o.pile_row_digests()       # (fnv, sum) of EVERY pile's data_ (round 6)
    # coverage vectors of a sample of live reads and of every read with pits / hills
    alive = np.nonzero(st["piles0"]["alive"])[0]
    rng = np.random.default_rng(0)
    pick = set(rng.choice(alive, size=min(n_data, len(alive)), replace=False).tolist()) if len(alive) else set()
    for key in ("pits0", "hills0"):
        offs = st[key][0]
        pick.update(int(x) for x in np.nonzero(offs[1:] > offs[:-1])[0][:32])
    pick.update(int(r) for r in data_of)
    st["data0"] = {r: o.pile_data(r) for r in sorted(pick)}
    if rc != 0:
        return st
    o.pass2()
    o.preprocess_chimeras()
    st["piles2"] = o.piles()
    st["ov"] = o.overlap_list(0)
    st["int"] = o.overlap_list(1)
    o.build_graph()
    st["nodes"] = o.nodes()
    if with_tr:
        st["n_tr"] = o.remove_transitive_edges()
    st["edges"] = o.edges()
    return st


_crafted = {}


def crafted_stages(case, n_threads=8, row_of=None):
    """The oracle on a case of tests/compcase.py or tests/containcase.py (rows: row_of(case, r), else the case's own row_of, else
    compcase's): the first pass, then every read's crafted row in place of its pile, and the
    per-pile annotation of Graph::initialize (graph.cpp:387-403) on it: find_valid_region - which leaves a live read's region
    [0, length) as it is, no value of its row is below 4, and takes the pile of a read that is to be dead, whose row is all zero -
    find_median, find_chimeric_hills, find_chimeric_pits.  Then the snapshot rala_hip_import_state takes, then the stages of
    oracle_stages.  Computed once per case and never changed."""
    import compcase
    if case.name in _crafted:
        return _crafted[case.name]
    row_of = row_of or getattr(case, "row_of", None) or compcase.row_of
    o = Oracle(case.read_len, case.overlaps, n_threads=n_threads)
    o.pass1()
    for r in range(case.n_reads):
        o.set_pile_state(r, row_of(case, r), 0, int(case.read_len[r]))
    st = {"init_rc": o.annotate()}    # (the oracle itself, with every row, is let go when this returns)
    assert st["init_rc"] == 0
    st["valid"] = o.valid()
    st["piles0"] = o.piles()
    st["pits0"] = o.all_intervals(0)
    st["hills0"] = o.all_intervals(1)
    o.pass2()
    st["alive_pass2"] = o.piles()["alive"]
    st["ov_pass2"] = o.overlap_list(0)
    st["int_pass2"] = o.overlap_list(1)
    o.preprocess_chimeras()
    st["piles2"] = o.piles()
    st["ov"] = o.overlap_list(0)
    st["int"] = o.overlap_list(1)
    o.build_graph()
    st["nodes"] = o.nodes()
    st["n_tr"] = o.remove_transitive_edges()
    st["edges"] = o.edges()
    _crafted[case.name] = st
    return st


def assert_same(name, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (name, a.shape, b.shape)
    if not (a == b).all():
        bad = np.nonzero(a != b)
        first = tuple(int(x[0]) for x in bad)
        raise AssertionError("%s: %d mismatches, first at %s: hip=%s oracle=%s" %
                             (name, len(bad[0]), first, a[first], b[first]))


def check_initialize(ctx, st, ds):
    """HIP state after rala_hip_initialize against the oracle snapshot."""
    assert_same("valid", ctx.valid(), st["valid"])
    hp = ctx.piles()
    op = st["piles0"]
    for k in ("alive", "begin", "end", "median", "p10"):
        assert_same("piles0." + k, hp[k], op[k])
    pit_aux = None
    for kind, key in ((0, "pits0"), (1, "hills0")):
        offs, pairs, aux = ctx.intervals(kind)
        assert_same(key + ".offsets", offs, st[key][0])
        assert_same(key + ".pairs", pairs, st[key][1])
        if kind == 0:
            pit_aux = aux
    for r, want in st["data0"].items():
        assert_same("pile_data[%d]" % r, ctx.pile_data(r), want)
    # the minimum the pile kernels record with every pit - the left side of `minimum * 1.84 <= component median` in
    # break_pits_kernel - is the row's minimum over [first, second], both ends inclusive: the positions the lambda of
    # Pile::break_over_chimeric_pits walks (reference pile.cpp:368-375); the kernels take the same range (pile_kernels.hip and
    # pile_runs_kernel.hip, where a pit is published), so no other one has to be argued equivalent
    offs, pairs = st["pits0"]
    for r, want in st["data0"].items():
        for k in range(int(offs[r]), int(offs[r + 1])):
            first, second = int(pairs[k][0]), int(pairs[k][1])
            low = int(want[first:second + 1].min())
            assert int(pit_aux[k]) == low, "pit %d of read %d, [%d, %d]: recorded minimum %d, the row's is %d" % (
                k - int(offs[r]), r, first, second, int(pit_aux[k]), low)
    # every row, hashed and summed where it lies (rala_hip_get_pile_row_digests) against the same vectors from the oracle's objects
    if "rows0" in st:
        fnv, inside, outside = ctx.pile_row_digests()
        assert_same("rows0.fnv", fnv, st["rows0"][0])
        assert_same("rows0.sum", inside, st["rows0"][1])
        assert not outside.any(), "values stored outside a valid region right after initialize"


def check_construct(ctx, st):
    hp = ctx.piles()
    op = st["piles2"]
    for k in ("alive", "begin", "end", "median"):
        assert_same("piles2." + k, hp[k], op[k])
    for which, key in ((0, "ov"), (1, "int")):
        h = ctx.overlap_list(which)
        o = st[key]
        assert_same(key + ".src", h["src"], o["src"].astype(np.uint32))
        for f in ("a_begin", "a_end", "b_begin", "b_end", "length", "type"):
            assert_same(key + "." + f, h[f], o[f])
    g = ctx.graph()
    assert_same("nodes", g["node_read"], st["nodes"])
    for f in ("src", "dst", "len"):
        assert_same("edges." + f, g[f], st["edges"][f])


def check_tr(ctx, st):
    n = ctx.remove_transitive_edges()
    g = ctx.graph()
    assert n == st["n_tr"], (n, st["n_tr"])
    assert_same("edges.marked", g["marked"], st["edges"]["marked"])


def run_hip(ctx, ds, construct=True):
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    if construct:
        ctx.construct()
