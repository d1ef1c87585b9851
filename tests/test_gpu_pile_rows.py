"""GPU: piles without resident rows (option pile_rows = 0).

rala_hip_initialize allocates no rows and its kernels store none; a row is rebuilt from the read's bound events by
pile_rows_kernel.hip whenever a getter, the digests or the sensitive pass' position-space fallback asks.  That kernel shares
nothing with the kernels that compute the annotations, so the digests below compare TWO implementations of the coverage with
the oracle: the annotations come from the run-space / position-space kernels, the rows from the materialiser.

Every case sets pile_rows = 0 and asks rala_hip_get_pile_rows_info for resident_bytes == 0."""
import functools
import os
import subprocess

import numpy as np
import pytest

from rala_amd.synth import Dataset

import golden_check as gc
import parity
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

T = 8192        # the materialiser's tile (kernels.h: kRowsTile)

OPTION_SETS = [{}, {"use_run_kernel": 0}, {"use_partitioned_buckets": 0}, {"use_fixed_buckets": 0},
               {"debug_force_big": 1, "debug_big_caps": (4 << 32) | 4}]
SETS = ["3000", "600", "c1", "plain", "sparse", "dense", "crafted"]


def fnv1a(data):
    h = 1469598103934665603
    for b in np.ascontiguousarray(data, dtype=np.uint16).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


class _Inputs:
    def __init__(self, read_len, overlaps):
        self.read_len, self.overlaps, self.n_reads = read_len, overlaps, len(read_len)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "3000":
        return Dataset(3000, 600_000, 21, 15)
    if name == "600":
        return Dataset(600, 60_000, 9, 15)
    if name == "crafted":
        _g, read_len, ov = gc.crafted_inputs()
        return _Inputs(read_len, ov)
    return gc.dataset_for(gc.load(name))


@functools.lru_cache(maxsize=None)
def stages(name):
    """the oracle's stages, computed once per data set and left unchanged; rows2: the digests under the final regions"""
    ds = inputs(name)
    st = parity.oracle_stages(ds, ref=ora.have_ref())
    if st["init_rc"] == 0:
        st["rows2"] = st["oracle"].pile_row_digests()
    return st


def rowless(factory, options=None, rows=0):
    ctx = factory()
    ctx.set_option("pile_rows", rows)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    return ctx


def assert_rowless(ctx):
    resident, _made = ctx.pile_rows_info()
    assert resident == 0, resident


def check_rows(ctx, want, after_initialize=False):
    fnv, inside, outside = ctx.pile_row_digests()
    parity.assert_same("row fnv", fnv, want[0])
    parity.assert_same("row sum", inside, want[1])
    assert not outside.any()            # nothing is stored, so nothing is stored outside a region
    return fnv


def test_default_keeps_the_rows_resident(hip_ctx_factory):
    ds = inputs("600")
    ctx = hip_ctx_factory()
    parity.run_hip(ctx, ds, construct=False)
    resident, made = ctx.pile_rows_info()
    assert resident >= 2 * int(ds.read_len.astype(np.uint64).sum()) and made == 0
    ctx.pile_data(0)
    ctx.pile_row_digests()
    assert ctx.pile_rows_info()[1] == 0
    # the option is read by initialize: the rows of the earlier call are given back
    ctx.set_option("pile_rows", 0)
    ctx.initialize()
    assert ctx.pile_rows_info() == (0, 0)
    ctx.pile_data(0)
    assert ctx.pile_rows_info() == (0, 1)


@pytest.mark.parametrize("options", OPTION_SETS)
@pytest.mark.parametrize("name", SETS)
def test_every_stage_and_every_row_matches_the_oracle(hip_ctx_factory, name, options):
    ds, st = inputs(name), stages(name)
    ctx = rowless(hip_ctx_factory, options)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    if st["init_rc"] != 0:
        # every read is filtered (the crafted set): EFILTERED is the reference's exit(1); what there is to compare is compared
        with pytest.raises(Exception) as e:
            ctx.initialize()
        assert getattr(e.value, "code", 0) == -4
        parity.assert_same("valid", ctx.valid(), st["valid"])
        check_rows(ctx, st["rows0"])
        assert_rowless(ctx)
        return
    ctx.initialize()
    assert_rowless(ctx)
    parity.check_initialize(ctx, st, ds)            # (every row: fnv, inside; 64 + rows element-wise)
    fnv = check_rows(ctx, st["rows0"])
    p = ctx.piles()
    alive = np.nonzero(p["alive"])[0]
    picked = alive[:: max(1, len(alive) // 12)][:12]
    for r in picked:
        row = ctx.pile_data(int(r))
        assert int(fnv[r]) == fnv1a(row), int(r)
        if int(r) in st["data0"]:
            parity.assert_same("pile_data[%d]" % r, row, st["data0"][int(r)])
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    check_rows(ctx, st["rows2"])
    assert_rowless(ctx)
    assert ctx.pile_rows_info()[1] >= 2 * ds.n_reads


def _snapshot(ctx, all_rows):
    out = {"piles": ctx.piles(), "pits": ctx.intervals(0), "hills": ctx.intervals(1), "valid": ctx.valid()}
    if all_rows:
        out["rows"] = {int(r): ctx.pile_data(int(r)) for r in np.nonzero(out["piles"]["alive"])[0]}
    return out


def _same_snapshot(a, b, what):
    for k in a["piles"]:
        parity.assert_same("%s piles.%s" % (what, k), a["piles"][k], b["piles"][k])
    for key in ("pits", "hills"):
        for i, part in enumerate(("offsets", "pairs", "aux")):
            parity.assert_same("%s %s.%s" % (what, key, part), a[key][i], b[key][i])
    parity.assert_same(what + " valid", a["valid"], b["valid"])
    if "rows" in a:
        assert a["rows"].keys() == b["rows"].keys()
        for r in a["rows"]:
            parity.assert_same("%s pile_data[%d]" % (what, r), a["rows"][r], b["rows"][r])


@pytest.mark.parametrize("name", [s for s in SETS if s != "crafted"])
def test_resident_and_rowless_contexts_agree(hip_ctx_factory, name):
    ds = inputs(name)
    got = []
    for rows in (1, 0):
        ctx = rowless(hip_ctx_factory, rows=rows)
        ctx.set_reads(ds.read_len)
        ctx.set_overlaps(ds.overlaps)
        ctx.initialize()
        snap = {"init": _snapshot(ctx, name == "600")}
        ctx.construct()
        snap["construct"] = _snapshot(ctx, name == "600")
        snap["lists"] = [ctx.overlap_list(w) for w in (0, 1)]
        snap["n_tr"] = ctx.remove_transitive_edges()
        snap["graph"] = ctx.graph()
        snap["digests"] = ctx.pile_row_digests()
        if rows == 0:
            assert_rowless(ctx)
        got.append(snap)
        ctx.close()
    a, b = got
    _same_snapshot(a["init"], b["init"], "initialize")
    _same_snapshot(a["construct"], b["construct"], "construct")
    for w in (0, 1):
        for f in a["lists"][w]:
            parity.assert_same("list %d.%s" % (w, f), a["lists"][w][f], b["lists"][w][f])
    assert a["n_tr"] == b["n_tr"]
    for f in a["graph"]:
        parity.assert_same("graph." + f, a["graph"][f], b["graph"][f])
    parity.assert_same("fnv", a["digests"][0], b["digests"][0])
    parity.assert_same("inside", a["digests"][1], b["digests"][1])


# ---- kernel boundaries -------------------------------------------------------------------------------------------------
def _long_and_dense(k):
    from test_gpu_parity import _Scaled
    return (lambda: _Scaled(Dataset(1500, 300_000, 11), 3), lambda: _Scaled(Dataset(800, 160_000, 5), 7), lambda: Dataset(1200, 24_000, 3))[k]()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_long_reads_and_event_dense_reads(hip_ctx_factory, k):
    """reads beyond 16384 / 32768 bases, reads with more events than 512 / 1024: every tier of the chain without rows"""
    ds = _long_and_dense(k)
    o = ora.Oracle(ds.read_len, ds.overlaps, n_threads=8, ref=ora.have_ref())
    assert o.initialize() == 0
    ctx = rowless(hip_ctx_factory)
    parity.run_hip(ctx, ds, construct=False)
    assert_rowless(ctx)
    hp, op = ctx.piles(), o.piles()
    for f in ("alive", "begin", "end", "median", "p10"):
        parity.assert_same("piles0." + f, hp[f], op[f])
    for kind in (0, 1):
        offs, pairs, _aux = ctx.intervals(kind)
        want = o.all_intervals(kind)
        parity.assert_same("intervals.offsets", offs, want[0])
        parity.assert_same("intervals.pairs", pairs, want[1])
    check_rows(ctx, o.pile_row_digests())


def add_layers(n, bounds):
    """Pile::add_layers (reference pile.cpp:274-297) over sorted bounds pos << 1 | is_end, uint16 with wrap-around"""
    row = np.zeros(n, dtype=np.uint16)
    cov, last = 0, 0
    for b in sorted(int(x) for x in bounds):
        pos = b >> 1
        if cov and pos > last:
            row[last:min(pos, n)] += np.uint16(cov)
        last = pos
        cov = (cov + (-1 if b & 1 else 1)) & 0xFFFF
    return row


def handmade():
    """read lengths around the materialiser's tile, one beyond 65536 bases, a read without events, a dead read, events at
    position 0 and at len, an overlap inside one tile, an overlap across three tiles - as bound tuples (what an owner context
    of a sharded run is given), since an overlap's bounds are drawn in by 15 bases and never lie at 0 or len"""
    lens = [T - 1, T, T + 1, 2 * T + 1, 70_001, 5000, 3000, 3 * T + 77]
    reads, bounds = [], []

    def cover(r, b, e, k=1):
        for _ in range(k):
            reads.extend([r, r])
            bounds.extend([b << 1, e << 1 | 1])
    for r, n in enumerate(lens):
        if r == 5:
            continue                    # no events
        if r == 6:
            cover(r, 100, 2000, 2)      # never four deep: dead
            continue
        cover(r, 0, n, 5)               # events at position 0 and at len
        cover(r, 15, n - 15, 2)
        cover(r, n // 2, n // 2 + 40)   # begins and ends inside one tile
        cover(r, 1, 2)
    cover(7, T - 3, 3 * T + 5, 3)       # spans three tiles (and both of their boundaries)
    cover(3, T, 2 * T)                  # events on the tile boundaries themselves
    cover(3, T - 1, 2 * T + 1)
    cover(4, 65_535, 65_537, 2)
    return np.array(lens, dtype=np.uint32), np.array(reads, dtype=np.uint32), np.array(bounds, dtype=np.uint32)


@pytest.mark.parametrize("options", [{}, {"use_fixed_buckets": 0}, {"use_run_kernel": 0}])
def test_handmade_rows_on_the_tile_boundaries(hip_ctx_factory, options):
    lens, reads, bounds = handmade()
    got = []
    for rows in (1, 0):
        ctx = rowless(hip_ctx_factory, options, rows=rows)
        ctx.set_reads(lens)
        ctx.set_bound_tuples(reads, bounds)
        ctx.initialize()
        p = ctx.piles()
        got.append((p, ctx.pile_row_digests(), [ctx.pile_data(r) for r in range(len(lens))]))
        if rows == 0:
            assert_rowless(ctx)
    (p1, d1, rows1), (p0, d0, rows0) = got
    for f in p1:
        parity.assert_same("piles." + f, p0[f], p1[f])
    assert list(p0["alive"]) == [1, 1, 1, 1, 1, 0, 0, 1]
    parity.assert_same("fnv", d0[0], d1[0])
    parity.assert_same("inside", d0[1], d1[1])
    for r, n in enumerate(lens):
        want = add_layers(int(n), bounds[reads == r])
        if p0["alive"][r]:
            want[:p0["begin"][r]] = 0
            want[p0["end"][r]:] = 0
            parity.assert_same("resident row %d" % r, rows1[r], want)
            assert int(d0[0][r]) == fnv1a(want)
        parity.assert_same("rebuilt row %d" % r, rows0[r], want)


def test_wrapped_coverage(hip_ctx_factory):
    """rows that hold (0 - k) mod 2^16 (tests/wrapcase.py)"""
    import wrapcase

    read_len, ov, _kinds = wrapcase.wrap_inputs(seed=1)
    o = ora.Oracle(read_len, ov, n_threads=4, ref=ora.have_ref())
    assert o.initialize() == 0
    want = o.pile_row_digests()
    for run_kernel in (1, 0):
        ctx = rowless(hip_ctx_factory, {"use_run_kernel": run_kernel})
        ctx.set_reads(read_len)
        ctx.set_overlaps(ov)
        ctx.initialize()
        assert_rowless(ctx)
        fnv = check_rows(ctx, want)
        alive = np.nonzero(ctx.piles()["alive"])[0]
        for r in alive[:4]:
            row = ctx.pile_data(int(r))
            parity.assert_same("pile_data[%d]" % r, row, o.pile_data(int(r)))
            assert int(fnv[r]) == fnv1a(row)


def test_saw_tooth_piles(hip_ctx_factory):
    """lists that outgrow every fixed capacity (tests/sawcase.py): the reads that run again with their lists in global memory"""
    import sawcase

    ds = sawcase.SawData([("pits", 300, 100, 50), ("hills", 130, 120, 40)], base=Dataset(400, 20_000, 5))
    o = ora.Oracle(ds.read_len, ds.overlaps, n_threads=4, ref=ora.have_ref())
    assert o.initialize() == 0
    ctx = rowless(hip_ctx_factory)
    parity.run_hip(ctx, ds, construct=False)
    assert_rowless(ctx)
    hp, op = ctx.piles(), o.piles()
    for f in ("alive", "begin", "end", "median", "p10"):
        parity.assert_same("piles0." + f, hp[f], op[f])
    for kind in (0, 1):
        offs, pairs, _aux = ctx.intervals(kind)
        want = o.all_intervals(kind)
        parity.assert_same("intervals.offsets", offs, want[0])
        parity.assert_same("intervals.pairs", pairs, want[1])
    check_rows(ctx, o.pile_row_digests())
    for r in ds.targets:
        parity.assert_same("pile_data[%d]" % r, ctx.pile_data(r), o.pile_data(r))


# ---- the scratch ---------------------------------------------------------------------------------------------------------
def test_digests_in_batches(hip_ctx_factory):
    """pile_rows_scratch_mb: the 3000-read set (46 MB of rows) in batches of 8 MB, and of 0 MB - a scratch smaller than any
    row, which grows to the longest one: a read per batch or a few"""
    ds = inputs("3000")
    want = stages("3000")["rows0"]
    total = int(((ds.read_len.astype(np.uint64) + 63) // 64 * 64).sum()) * 2
    assert total > 3 * (8 << 20)
    single = None
    for mb in (256, 8, 0):
        ctx = rowless(hip_ctx_factory, {"pile_rows_scratch_mb": mb})
        parity.run_hip(ctx, ds, construct=False)
        got = ctx.pile_row_digests()
        assert_rowless(ctx)
        assert ctx.pile_rows_info()[1] == ds.n_reads
        if single is None:
            single = got
            check_rows(ctx, want)
        for k in range(3):
            parity.assert_same("digest %d at %d MB" % (k, mb), got[k], single[k])
        ctx.close()


# ---- the sensitive pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{}, {"use_run_kernel": 0}, {"use_gpu_tail": 0}])
def test_sensitive_pass_without_rows(hip_ctx_factory, options):
    """rala -s: medians and repeat hills against the oracle and the resident mode - as it is, and with every target on the
    position-space fallback (use_run_kernel = 0: pile_repeats_kernel on rows rebuilt in the scratch); the rows of all targets
    hold the second add_layers afterwards"""
    ds = Dataset(5000, 1_000_000, 7)
    o = ora.Oracle(ds.read_len, ds.overlaps, n_threads=8)
    assert o.initialize() == 0
    o.pass2()
    o.preprocess_chimeras()
    p = o.piles()
    sens = ds.sensitive(p["alive"], p["begin"], p["end"])
    o.preprocess_repeats(sens)
    want_rep, want_p = o.all_intervals(2), o.piles()
    want_rows = o.pile_row_digests()
    targets = np.unique(sens.b_id)
    got = []
    for rows in (1, 0):
        ctx = rowless(hip_ctx_factory, options, rows=rows)
        parity.run_hip(ctx, ds, construct=False)
        ctx.construct(sens)
        offs, pairs, flags = ctx.intervals(2)
        parity.assert_same("rep.offsets", offs, want_rep[0])
        parity.assert_same("rep.pairs", pairs, want_rep[1])
        assert len(pairs) > 0
        hp = ctx.piles()
        for f in ("alive", "begin", "end", "median", "p10"):
            parity.assert_same("piles." + f, hp[f], want_p[f])
        fnv, inside, _outside = ctx.pile_row_digests()
        parity.assert_same("row fnv of the targets", fnv[targets], want_rows[0][targets])
        parity.assert_same("row sum of the targets", inside[targets], want_rows[1][targets])
        for r in targets[:8]:
            parity.assert_same("pile_data[%d]" % r, ctx.pile_data(int(r)), o.pile_data(int(r)))
        if rows == 0:
            assert_rowless(ctx)
            # one sensitive construct per initialize: its bounds are what the rows are rebuilt from
            with pytest.raises(Exception) as e:
                ctx.construct(sens)
            assert getattr(e.value, "code", 0) == -2
        got.append((fnv, inside, flags, ctx.graph()))
        ctx.close()
    for k in range(3):
        parity.assert_same("resident against rowless %d" % k, got[0][k], got[1][k])
    for f in got[0][3]:
        parity.assert_same("graph." + f, got[0][3][f], got[1][3][f])


# ---- sharded runs ----------------------------------------------------------------------------------------------------------
def _owner(rank):
    """the context that holds a rank's rows (borrowed): it takes the options that concern them, as pile_chunk_mb"""
    from rala_amd import hip
    return hip.Context(_borrowed=rank.L.rala_hip_mg_owner_context(rank.h))


def test_sharded_run_with_rowless_owners():
    from test_gpu_sharded import Sharded

    world = 3
    ds = Dataset(3000, 600_000, 21, 31)
    o = ora.Oracle(ds.read_len, ds.overlaps, n_threads=8, ref=ora.have_ref())
    assert o.construct() == 0
    want_fnv, want_sum = o.pile_row_digests()
    sh = Sharded(ds, world)
    try:
        for r in sh.ranks:
            _owner(r).set_option("pile_rows", 0)
        sh.run()
        fnv = np.zeros(ds.n_reads, dtype=np.uint64)
        tot = np.zeros(ds.n_reads, dtype=np.uint64)
        for k, r in enumerate(sh.ranks):
            f, s, out = r.pile_row_digests()
            fnv[k::world] = f
            tot[k::world] = s
            assert not out.any()
            assert _owner(r).pile_rows_info()[0] == 0
        parity.assert_same("row fnv", fnv, want_fnv)
        parity.assert_same("row sum", tot, want_sum)
        alive = np.nonzero(o.piles()["alive"])[0]
        for r in alive[:: max(1, len(alive) // 12)]:
            row = sh.ranks[int(r) % world].pile_data(int(r))
            parity.assert_same("pile_data[%d]" % r, row, o.pile_data(int(r)))
    finally:
        sh.close()


def test_sharded_rows_that_straddle_two_chunks(hip_ctx_factory):
    """the default (resident) rows in chunks of 2 MB on the owners: every row through rala_hip_mg_get_pile_data - a row that
    lies across two mapped chunks is copied chunk by chunk - equals the single context's"""
    from test_gpu_sharded import Sharded

    world = 3
    ds = Dataset(3000, 600_000, 21, 31)
    ctx = hip_ctx_factory()
    parity.run_hip(ctx, ds)
    alive = ctx.piles()["alive"]
    sh = Sharded(ds, world)
    try:
        for r in sh.ranks:
            _owner(r).set_option("pile_chunk_mb", 2)
        sh.run()
        for r in range(ds.n_reads):
            if alive[r]:
                parity.assert_same("pile_data[%d]" % r, sh.ranks[r % world].pile_data(r), ctx.pile_data(r))
    finally:
        sh.close()


# ---- full size --------------------------------------------------------------------------------------------------------------
def test_fullsize_c2_without_rows(hip_ctx_factory):
    """C2 (tests/golden/fullsize_c2.json, the digests of the reference objects' result) with pile_rows = 0, under the assertion
    test_gpu_fullsize.py makes for it: every stage's digest - rows0 / rows2 and their sums among them, i.e. every row rebuilt and
    hashed in batches of the default 256 MB scratch - and the product launch shape of the first kernel without its row stores"""
    import test_gpu_fullsize as fs

    want = fs.load_digests("c2")
    ds = fs.dataset("c2")
    assert (ds.n_reads, len(ds.overlaps)) == (want["n_reads"], want["n_overlaps"])
    ctx = fs.run(hip_ctx_factory, ds, pile_rows=0)
    assert_rowless(ctx)
    got = fs.stage_digests(ctx)
    for k, v in got.items():
        assert v == want[k], "c2: stage %s differs from the oracle" % k
    assert {"rows0", "rows0_sum", "rows2", "rows2_sum"} <= set(got)
    assert_rowless(ctx)
    assert ctx.pile_rows_info()[1] >= 2 * ds.n_reads


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_cli_without_rows(tmp_path):
    """RALA_PILE_ROWS=0 rala -d prefix ...: byte-identical contigs and debug files (the small set of test_gpu_cli.py)"""
    from rala_amd import build

    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(600, 120_000, 17)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    outs = []
    for k, env in enumerate(({}, {"RALA_PILE_ROWS": "0"})):
        d = tmp_path / ("run%d" % k)
        d.mkdir()
        res = subprocess.run([exe, "-u", "-d", str(d / "dbg"), fa, paf], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE)
        assert res.returncode == 0, res.stderr.decode()
        files = {f.name: f.read_bytes() for f in sorted(d.iterdir())}
        assert files, "no debug files"
        outs.append((res.stdout, files))
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) > 0
    assert outs[0][1].keys() == outs[1][1].keys()
    for name in outs[0][1]:
        assert outs[0][1][name] == outs[1][1][name], name
