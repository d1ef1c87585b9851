"""The life of one librala_hip context through the C ABI (needs an MI355X): which call is allowed in which state and what the
others are told, one context used for several data sets and several kinds of input, state installed over old results, inputs
dropped by a failed ingest, a data set whose reads are all filtered.

The flags behind all this live in rala_amd/csrc/lifecycle.h ("The life of a context").  Everything here is what
the library did before those flags had one home: return codes, the texts of rala_hip_last_error, results.
"""
import numpy as np
import pytest

from rala_amd import hip
from rala_amd.synth import Dataset, Overlaps, FIELDS

import parity

pytestmark = pytest.mark.gpu

EINVAL, EFILTERED = -2, -4

_made = {}


def _data(name):
    """the two data sets (different read and overlap counts: every buffer shrinks and grows) and their oracle stages, made once"""
    if name not in _made:
        ds = Dataset(400, 20_000, 5) if name == "A" else Dataset(1000, 200_000, 1)
        _made[name] = (ds, parity.oracle_stages(ds))
    return _made[name]


def _sensitive(name):
    """the oracle's run with a sensitive set (as _check_sensitive of test_gpu_parity.py), made once"""
    key = name + "+sens"
    if key not in _made:
        from oracle.oracle import Oracle

        ds = _data(name)[0]
        o = Oracle(ds.read_len, ds.overlaps, n_threads=8)
        assert o.initialize() == 0
        o.pass2()
        o.preprocess_chimeras()
        p = o.piles()
        sens = ds.sensitive(p["alive"], p["begin"], p["end"])
        o.preprocess_repeats(sens)
        want = {"sens": sens, "rep": o.all_intervals(2), "ov": o.overlap_list(0), "piles": o.piles()}
        o.build_graph()
        want["n_tr"] = o.remove_transitive_edges()
        want["edges"] = o.edges()
        _made[key] = want
    return _made[key]


def _run(ctx, name, sens=False):
    """one data set from its reads to the transitive marks on ctx, every stage against the oracle"""
    ds, st = _data(name)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    if not sens:
        ctx.construct()
        parity.check_construct(ctx, st)
        parity.check_tr(ctx, st)
        assert len(ctx.intervals(2)[1]) == 0        # (no repeat hills without a sensitive set, whatever the context ran before)
        return
    want = _sensitive(name)
    ctx.construct(want["sens"])
    offs, pairs, _ = ctx.intervals(2)
    parity.assert_same("rep.offsets", offs, want["rep"][0])
    parity.assert_same("rep.pairs", pairs, want["rep"][1])
    hp = ctx.piles()
    for k in ("alive", "begin", "end", "median", "p10"):
        parity.assert_same("piles." + k, hp[k], want["piles"][k])
    parity.assert_same("ov.src", ctx.overlap_list(0)["src"], want["ov"]["src"].astype(np.uint32))
    assert ctx.remove_transitive_edges() == want["n_tr"]
    g = ctx.graph()
    for k in ("src", "dst", "len", "marked"):
        parity.assert_same("edges." + k, g[k], want["edges"][k])


# ---- refusals ------------------------------------------------------------------------------------------------------------

NOT_INITIALIZED = {
    "construct": "rala_hip_initialize must succeed first",
    "tr": "rala_hip_construct must succeed first",
    "valid": "run rala_hip_dedupe or rala_hip_initialize first",
    "piles": "not initialized",
    "intervals": "not initialized",
    "pile_data": "bad read / not initialized",
    "row_digests": "not initialized",
    "device_state": "not initialized",
    "find_hills": "bad read / not initialized",
    "overlap_list": "not constructed",
    "graph": "not constructed",
}
NOT_CONSTRUCTED = {k: NOT_INITIALIZED[k] for k in ("tr", "overlap_list", "graph")}
# Where the context held overlaps with validity bits before and holds none now (a failed ingest, bound tuples set), the bits are
# not refused - as before this file: rala_hip_get_valid copies none, there are no overlaps.  Only rala_hip_set_overlaps takes them away.
NOT_INITIALIZED_BITS_KEPT = {k: v for k, v in NOT_INITIALIZED.items() if k != "valid"}


def _calls(ctx):
    """every stage and getter; the ones whose Python wrapper sizes a buffer from what the wrapper was told go to the library directly"""
    buf = np.zeros(1 << 16, dtype=np.uint64)
    return {
        "initialize": ctx.initialize,
        "dedupe": ctx.dedupe,
        "construct": ctx.construct,
        "tr": ctx.remove_transitive_edges,
        "valid": lambda: ctx._check(ctx.L.rala_hip_get_valid(ctx.h, buf.ctypes.data)),
        "piles": ctx.piles,
        "intervals": lambda: ctx.intervals(0),
        "pile_data": lambda: ctx._check(ctx.L.rala_hip_get_pile_data(ctx.h, 0, buf.ctypes.data)),
        "row_digests": ctx.pile_row_digests,
        "device_state": ctx.device_state,
        "find_hills": lambda: ctx.find_repetitive_hills(0, 0, 100, 10, 5, 10),
        "overlap_list": lambda: ctx.overlap_list(0),
        "graph": ctx.graph,
    }


def _refused(ctx, fn, text, code=EINVAL):
    with pytest.raises(hip.RalaHipError) as e:
        fn()
    got = ctx.L.rala_hip_last_error(ctx.h).decode()
    assert (e.value.code, got) == (code, text)


def _all_refused(ctx, state, table):
    calls = _calls(ctx)
    for name, text in table.items():
        try:
            _refused(ctx, calls[name], text)
        except BaseException as e:
            raise AssertionError("state '%s', call '%s': %s" % (state, name, e)) from None


def test_refusals_in_every_state(hip_ctx_factory):
    ds, st = _data("B")
    ctx = hip_ctx_factory()
    # created
    no_reads = dict(NOT_INITIALIZED, initialize="no reads set", dedupe="no reads set")
    _all_refused(ctx, "created", no_reads)
    _refused(ctx, lambda: ctx.set_bound_tuples(np.zeros(2), np.zeros(2)), "no reads set")
    one = dict(begin=[0], end=[1], median=[1], p10=[1], alive=[1])
    none = (np.zeros(2, dtype=np.uint64), np.zeros((0, 2)), np.zeros(0))
    _refused(ctx, lambda: ctx.import_state(np.zeros(0), one, none, none), "no reads set")
    # reads set
    ctx.set_reads(ds.read_len)
    _all_refused(ctx, "reads set", dict(NOT_INITIALIZED, initialize="no overlaps or bound tuples set", dedupe="no overlaps set"))
    # inputs set
    ctx.set_overlaps(ds.overlaps)
    _all_refused(ctx, "inputs set", NOT_INITIALIZED)
    # initialized
    ctx.initialize()
    _all_refused(ctx, "initialized", NOT_CONSTRUCTED)
    _refused(ctx, lambda: ctx.intervals(3), "bad interval kind")
    parity.check_initialize(ctx, st, ds)
    # constructed
    ctx.construct()
    _all_refused(ctx, "constructed", {"construct": "object already constructed"})
    parity.check_construct(ctx, st)
    # transitive reduction done (it may be asked for again; construct may not)
    parity.check_tr(ctx, st)
    _all_refused(ctx, "reduced", {"construct": "object already constructed"})
    assert ctx.remove_transitive_edges() == st["n_tr"]
    # new overlaps on the constructed context: back to "inputs set", nothing of the old results can be asked for
    ctx.set_overlaps(ds.overlaps)
    _all_refused(ctx, "inputs set again", NOT_INITIALIZED)
    # ... and new reads: the overlaps stay the context's (either order of the two setters is allowed)
    ctx.set_reads(ds.read_len)
    _all_refused(ctx, "reads set again", NOT_INITIALIZED)
    ctx.initialize()
    _all_refused(ctx, "initialized again", NOT_CONSTRUCTED)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


def test_removed_measurement_option_is_unknown(hip_ctx_factory):
    """debug_pile_variant (the pile kernel's measurement variants, docs/history/experiments/r20_pile_ab_variants.patch) is refused
    like any unknown key, and the context goes on: it initializes a set of 8 reads and 16 overlaps"""
    ctx = hip_ctx_factory()
    _refused(ctx, lambda: ctx.set_option("debug_pile_variant", 0), "unknown option")
    # 8 reads of 10 000 bases; read r is the query of two overlaps, with r + 1 and r + 2, over [200, 9800) on both sides: every
    # read lies under four, each bound 15 bases further in (the oracle says the same)
    a = np.repeat(np.arange(8), 2)
    lo, hi = np.full(16, 200), np.full(16, 9800)
    ctx.set_reads(np.full(8, 10_000, dtype=np.uint32))
    ctx.set_overlaps(Overlaps(a_id=a, b_id=(a + np.tile([1, 2], 8)) % 8, a_begin=lo, a_end=hi, b_begin=lo, b_end=hi, length=hi - lo,
                              strand=np.zeros(16, dtype=np.uint8)))
    ctx.initialize()
    p = ctx.piles()
    for k, want in (("alive", 1), ("begin", 215), ("end", 9785), ("median", 4), ("p10", 4)):
        parity.assert_same("piles." + k, p[k], np.full(8, want, dtype=p[k].dtype))


# ---- one context, several data sets --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pile_rows", [1, 0])
def test_context_used_again(hip_ctx_factory, pile_rows):
    """A, B and A again with a sensitive set each (the repeat hills' arrays on the device, the sensitive bounds' CSR), B plain:
    buffers shrink and grow, and nothing of a round is seen by the next"""
    ctx = hip_ctx_factory()
    ctx.set_option("pile_rows", pile_rows)
    _run(ctx, "A")
    _run(ctx, "B", sens=True)
    _run(ctx, "A", sens=True)
    _run(ctx, "B")
    resident, _ = ctx.pile_rows_info()
    assert (resident != 0) == (pile_rows != 0)


# ---- one context, several kinds of input ---------------------------------------------------------------------------------

def _per_read(ctx):
    return ctx.piles(), ctx.intervals(0), ctx.intervals(1), ctx.pile_row_digests()


def _same_per_read(got, want):
    for k in want[0]:
        parity.assert_same("piles." + k, got[0][k], want[0][k])
    for which, name in ((1, "pits"), (2, "hills")):
        for k in range(3):
            parity.assert_same("%s[%d]" % (name, k), got[which][k], want[which][k])
    for k in range(3):
        parity.assert_same("row digests[%d]" % k, got[3][k], want[3][k])


def test_kind_of_input_switched(hip_ctx_factory):
    import torch

    b, _ = _data("B")
    ctx = hip_ctx_factory()
    _run(ctx, "A")
    # B's bounds as tuples, emitted by another context (what an owner of a sharded run is given)
    other = hip_ctx_factory()
    other.set_reads(b.read_len)
    other.set_overlaps(b.overlaps)
    n_tuples = 4 * len(b.overlaps)
    tuples = torch.empty(n_tuples, dtype=torch.int64, device="cuda:0")
    other.emit_bound_tuples(tuples.data_ptr())
    fresh = hip_ctx_factory()
    fresh.set_reads(b.read_len)
    fresh.set_bound_tuples_device(tuples.data_ptr(), n_tuples)
    fresh.initialize()
    want = _per_read(fresh)
    assert want[0]["alive"].any()
    ctx.set_reads(b.read_len)
    ctx.set_bound_tuples_device(tuples.data_ptr(), n_tuples)
    _all_refused(ctx, "tuples set", NOT_INITIALIZED_BITS_KEPT)
    ctx.initialize()
    _same_per_read(_per_read(ctx), want)
    # bounds alone make no graph, and the validity bits belong to overlaps
    tuple_mode = dict(NOT_CONSTRUCTED, construct="construct needs the overlaps (rala_hip_set_overlaps)", dedupe="no overlaps set",
                      valid="run rala_hip_dedupe or rala_hip_initialize first")
    _all_refused(ctx, "initialized from tuples", tuple_mode)
    # back to overlaps
    _run(ctx, "A")
    _run(ctx, "B")


# ---- state installed over old results ------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["host", "device"])
def test_state_installed_over_old_results(hip_ctx_factory, how):
    """rala_hip_import_state / _device on a context that has just constructed (its results on the device, the host's copies not
    fetched): what the getters return from then on is the installed state, and construct runs from it"""
    ds, st = _data("B")
    first = hip_ctx_factory()
    first.set_reads(ds.read_len)
    first.set_overlaps(ds.overlaps)
    first.initialize()
    pits, hills = first.intervals(0), first.intervals(1)
    ctx = hip_ctx_factory()
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    ctx.construct()
    assert ctx.remove_transitive_edges() == st["n_tr"]
    if how == "host":
        ctx.import_state(first.valid(), first.piles(), pits, hills)
    else:
        state = first.device_state()
        ctx.import_state_device(**{name: getattr(state, name) for name, _ in hip.DeviceState._fields_})
    _all_refused(ctx, "state installed", NOT_CONSTRUCTED)
    # (no rows came with the state)
    _all_refused(ctx, "state installed", {"pile_data": "piles live on the owning rank's context",
                                          "row_digests": "piles live on the owning rank's context",
                                          "find_hills": "the piles live on another context"})
    assert ctx.num_prefiltered() == first.num_prefiltered()
    parity.assert_same("valid", ctx.valid(), st["valid"])
    hp = ctx.piles()
    for k in ("alive", "begin", "end", "median", "p10"):
        parity.assert_same("piles0." + k, hp[k], st["piles0"][k])
    for kind, want in ((0, pits), (1, hills)):
        got = ctx.intervals(kind)
        for k in range(3):
            parity.assert_same("intervals(%d)[%d]" % (kind, k), got[k], want[k])
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


# ---- a failed ingest drops the inputs ------------------------------------------------------------------------------------

def test_failed_ingest_drops_the_inputs(hip_ctx_factory, tmp_path):
    ctx = hip_ctx_factory()
    _run(ctx, "B")
    ctx.set_name_table(np.zeros((1, 8), dtype=np.uint32), np.zeros(0, dtype=np.uint8))
    path = str(tmp_path / "no_such_file.paf")
    _refused(ctx, lambda: ctx.set_overlaps_from_paf(path), "cannot open " + path)
    _all_refused(ctx, "inputs dropped", dict(NOT_INITIALIZED_BITS_KEPT, initialize="no overlaps or bound tuples set", dedupe="no overlaps set"))
    ctx.valid()
    _run(ctx, "B")


def test_failed_sharded_ingest_drops_only_the_inputs(tmp_path):
    """The sharded runner's device ingest (rala_hip_mg_set_overlaps_from_mhap; a world of one) drops the slice context's inputs
    before it reads the file - and ONLY them: when the file cannot be opened, or is no file of records, the rank has no overlaps
    (rala_hip_mg_run and rala_hip_initialize are refused), while the results of the run before stay readable through
    rala_hip_mg_context.  (The single-context ingest above takes the results away too.)"""
    import ctypes

    ds, st = _data("B")
    group = hip.LocalGroup(1)
    rank = hip.ShardedRank(0, 0, 1, group)
    try:
        rank.set_reads(ds.read_len)
        rank.set_overlaps(ds.overlaps, 0)
        ctx = rank.context()

        def last_run_readable():
            parity.check_construct(ctx, st)
            parity.assert_same("edges.marked", ctx.graph()["marked"], st["edges"]["marked"])
            hp = ctx.piles()
            for k in ("alive", "begin", "end", "median"):
                parity.assert_same("piles2." + k, hp[k], st["piles2"][k])

        def ingest(path):
            bad, irregular = ctypes.c_int64(-1), ctypes.c_int(0)
            rc = rank.L.rala_hip_mg_set_overlaps_from_mhap(rank.h, ctypes.c_char_p(path.encode()), ctypes.c_int(0), ctypes.c_uint32(2),
                                                           ctypes.byref(bad), ctypes.byref(irregular))
            return rc, irregular.value

        def no_inputs(state):
            with pytest.raises(hip.RalaHipError) as e:
                rank.run()
            assert (e.value.code, rank.L.rala_hip_mg_last_error(rank.h).decode()) == (EINVAL, "set reads and overlaps first"), state
            _all_refused(ctx, state, {"initialize": "no overlaps or bound tuples set", "dedupe": "no overlaps set"})

        assert hip.run_ranks([rank]) == st["n_tr"]
        last_run_readable()
        # a file that is no file of records: nothing is set, the call itself succeeds
        text = tmp_path / "not_records.mhap"
        text.write_text("short line\n" * 3)
        rc, irregular = ingest(str(text))
        assert rc == 0 and irregular != 0
        no_inputs("irregular file")
        last_run_readable()
        # a file that is not there
        rc, irregular = ingest(str(tmp_path / "no_such_file.mhap"))
        assert rc == EINVAL
        no_inputs("no file")
        last_run_readable()
    finally:
        rank.close()
        group.close()


# ---- every read filtered -------------------------------------------------------------------------------------------------

def test_every_read_filtered(hip_ctx_factory):
    """rala_hip_initialize returns RALA_HIP_EFILTERED with the context INITIALIZED (the flag is set before that return): the
    getters answer, and construct runs on the nothing that is left"""
    ctx = hip_ctx_factory()
    ctx.set_reads(np.array([5000, 8000, 12000], dtype=np.uint32))
    ctx.set_overlaps(Overlaps(strand=np.zeros(0, np.uint8), **{f: np.zeros(0, np.uint32) for f in FIELDS}))
    _refused(ctx, ctx.initialize, "filtered all sequences", EFILTERED)
    assert ctx.num_prefiltered() == 3
    p = ctx.piles()
    for k in p:
        assert not p[k].any(), k
    ctx.construct()
    g = ctx.graph()
    assert len(g["node_read"]) == 0 and len(g["src"]) == 0
    assert len(ctx.overlap_list(0)["src"]) == 0
    assert ctx.remove_transitive_edges() == 0
    _all_refused(ctx, "constructed from nothing", {"construct": "object already constructed"})
    _run(ctx, "A")
