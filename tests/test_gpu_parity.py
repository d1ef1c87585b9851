"""Parity of the HIP hot path with the oracle, through the C ABI (needs an MI355X)."""
import numpy as np
import pytest

from rala_amd.synth import Dataset

import parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run_kernel", [1, 0])
@pytest.mark.parametrize("n,g,seed", [(1000, 200_000, 1), (3000, 600_000, 21), (5000, 1_000_000, 7),
                                      (2000, 1_200_000, 33), (400, 20_000, 5),
                                      (600, 60_000, 9),        # ~100x: reads beyond the 512-event cap
                                      (1500, 12_000, 3)])      # ~750x: beyond the 2048-event cap too
def test_full_path_small(hip_ctx_factory, n, g, seed, run_kernel):
    """run_kernel=1: run-space kernel (+ position-space kernel for event-dense reads);
    run_kernel=0: every read through the position-space kernel."""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_run_kernel", run_kernel)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    tm = ctx.timings()
    print(tm)
    if run_kernel and (n, g) == (1500, 12_000):
        assert tm["pile_position_reads"] > 0 and tm["pile_overflow_reads"] >= tm["pile_position_reads"]


@pytest.mark.parametrize("run_kernel", [1, 0])
@pytest.mark.parametrize("n,g,seed", [(3000, 3_000_000, 77), (6000, 2_500_000, 78)])
def test_heavy_tailed_read_lengths(hip_ctx_factory, n, g, seed, run_kernel):
    """Read lengths with a heavy tail (3 kb + exponential, some reads 30 - 90 kb longer: up to 105 kb) instead of the
    bell of the named configurations: every length class of the pile chain (16 384 / 32 768 / 65 535 bases and
    beyond), the 8-byte per-read records of the second pass, coverage from 11x to 27x."""
    ds = Dataset(n, g, seed, plants=31)
    assert (ds.read_len > 65535).sum() > 0 and (ds.read_len > 32768).sum() > 20 and (ds.read_len <= 16384).sum() > n // 2
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_run_kernel", run_kernel)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("n,g,seed", [(3000, 600_000, 21), (400, 20_000, 5), (1500, 12_000, 3)])
def test_bucketing_variants(hip_ctx_factory, n, g, seed):
    """The ways the bounds reach the pile kernel: the target side partitioned into an exact CSR (default,
    bucket_kernels.hip), fixed slots (the position inside the slot is what the counting atomic returns) and
    the exact CSR through count, scan, scatter."""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    # (use_side_stream = 0: duplicate removal and the pile chain's small kernels on the main stream)
    for opts in ({"use_fixed_buckets": 0}, {}, {"use_partitioned_buckets": 0}, {"use_side_stream": 0},
                 {"use_side_stream": 0, "use_partitioned_buckets": 0}, {"use_side_stream": 0, "use_fixed_buckets": 0}):
        ctx = hip_ctx_factory()
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_reads(ds.read_len)
        ctx.set_overlaps(ds.overlaps)
        ctx.initialize()
        parity.check_initialize(ctx, st, ds)


def _bound_events(ds):
    """events per read as the bucketing counts them: every overlap whose two names resolve puts a begin and an end on each
    of its reads"""
    ov, n = ds.overlaps, ds.n_reads
    ok = (ov.a_id < n) & (ov.b_id < n)
    return 2 * np.bincount(ov.a_id[ok], minlength=n) + 2 * np.bincount(ov.b_id[ok], minlength=n)


def test_fixed_slot_overflow_runs_again_on_the_exact_path(hip_ctx_factory):
    """A read with more bound events than a fixed slot holds (2048) on the fixed-slot path: rala_hip_initialize notices with
    its one look and runs once more through the exact CSR.  The smallest generated set of this family with such a read (one,
    2120 events: the assertion below guards that thin margin); every stage against the oracle, then a second call on the
    same context, then a set without such a read.  Parity cannot tell the exact path from the fixed slots, so this shows that
    the retry and what follows it on the context compute the right thing - not which path the later calls took."""
    ds = Dataset(520, 8_000, 5)
    ev = _bound_events(ds)
    assert (ev > 2048).sum() >= 1 and ev.max() < 2200, (int((ev > 2048).sum()), int(ev.max()))
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_partitioned_buckets", 0)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    small = Dataset(400, 20_000, 5)
    assert _bound_events(small).max() <= 2048
    st2 = parity.oracle_stages(small)
    ctx.set_reads(small.read_len)
    ctx.set_overlaps(small.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st2, small)
    ctx.construct()
    parity.check_construct(ctx, st2)
    parity.check_tr(ctx, st2)


@pytest.mark.parametrize("shift", [12, 13, 14])
@pytest.mark.parametrize("n,g,seed", [(40_000, 8_000_000, 13), (9000, 1_800_000, 4)])
def test_first_level_partition_sizes(hip_ctx_factory, n, g, seed, shift):
    """The partitioned bucketing's first-level partitions hold 4096 reads up to a million reads and 8192 / 16384 beyond (never
    more than 256 partitions - round 6: C5's first scatter wrote runs of four records over 977 of them); here every size on data
    sets of ten and three partitions of 4096 (option debug_part_shift), every pile row against the oracle's; the sharded owners'
    level-2 kernels see the same 14-bit record keys (tests/test_gpu_sharded.py, tests/fuzz_sharded.py)"""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("debug_part_shift", shift)           # (this context's own: nothing to put back)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("n,g,seed,window", [(40_000, 8_000_000, 13, 64), (9000, 1_800_000, 4, 7), (9000, 1_800_000, 4, 1)])
@pytest.mark.parametrize("sensitive", [False, True])
def test_counting_pass_in_windows(hip_ctx_factory, n, g, seed, window, sensitive):
    """The partitioned bucketing's counting pass keeps a histogram of all groups of 128 reads in a workgroup's LDS: 4.9 M reads.
    Beyond that (round 6) it counts window after window of groups, the ids streamed once per window; here with windows of 64 / 7 /
    1 groups on sets of 313 and 71 (option debug_count_window), duplicate removal's first pass riding on the first window only;
    the sensitive pass' records (group_count_records_kernel) the same way"""
    ds = Dataset(n, g, seed)
    if sensitive:
        if n <= 9000:       # (the option belongs to a context: to the one that runs the sensitive pass)
            _check_sensitive(hip_ctx_factory, ds, 1, 1, expect_hills=True, options={"debug_count_window": window})
        return
    ctx = hip_ctx_factory()
    ctx.set_option("debug_count_window", window)
    st = parity.oracle_stages(ds)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("n,g,seed", [(9000, 1_800_000, 4), (600, 60_000, 9)])
@pytest.mark.parametrize("chunk_mb", [2, 16, 0])
def test_rows_in_mapped_chunks(hip_ctx_factory, n, g, seed, chunk_mb):
    """The rows of all piles lie in physical chunks mapped side by side into one range (hipMemCreate / hipMemMap; 1 GB each in the
    product, where a data set has that much - round 6: the first pile kernel's stores are faster there than where one hipMalloc
    puts them); here chunks of 2 and 16 MB under sets of 180 and 12 MB of rows, and the single hipMalloc (0); the set given twice,
    the second time larger (the range is released and mapped again); every row read back (digests, Pile::data() of the samples)"""
    ctx = hip_ctx_factory()
    ctx.set_option("pile_chunk_mb", chunk_mb)
    for d in (Dataset(600, 60_000, seed), Dataset(n, g, seed)):
        st = parity.oracle_stages(d)
        ctx.set_reads(d.read_len)
        ctx.set_overlaps(d.overlaps)
        ctx.initialize()
        parity.check_initialize(ctx, st, d)
        ctx.construct()
        parity.check_construct(ctx, st)
        parity.check_tr(ctx, st)


@pytest.mark.parametrize("fail_at", [0, 3])
def test_rows_chunks_that_cannot_be_mapped(hip_ctx_factory, fail_at):
    """the mapping of the rows' chunks fails (at the first chunk; half way): what was created is unmapped and released, the rows
    come from one hipMalloc and the result is the same; the device's free memory afterwards is what it was"""
    import torch

    ds = Dataset(9000, 1_800_000, 4)
    st = parity.oracle_stages(ds)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ctx = hip_ctx_factory()
    ctx.set_option("pile_chunk_mb", 16)
    ctx.set_option("debug_chunk_fail", fail_at)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert abs(free0 - free1) < (64 << 20), (free0, free1)


@pytest.mark.parametrize("n,g,seed", [(9000, 1_800_000, 4), (600, 60_000, 9)])
@pytest.mark.parametrize("opts", [{}, {"use_run_kernel": 0}])
def test_row_offsets_in_events(hip_ctx_factory, n, g, seed, opts):
    """The partitioned bucketing's row offsets count bound PAIRS since round 6 (2^31 overlaps per context instead of 2^30; every
    other test runs that way); debug_ev_events = 1 is the old unit - both pile kernels read either (PileArgs::ev_shift)"""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("debug_ev_events", 1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("n,g,seed", [(3000, 600_000, 21), (5000, 1_000_000, 7), (600, 60_000, 9), (40_000, 8_000_000, 13)])
@pytest.mark.parametrize("opts", [{"debug_fp_lds_limit": 0}, {"debug_fp_lds_limit": 40}, {"use_round_batches": 0},
                                  {"debug_fp_lds_limit": 0, "debug_fp_give_up": 1},
                                  {"debug_fp_lds_limit": 0, "debug_fp_give_up": 2}])
def test_containment_fixed_point_variants(hip_ctx_factory, n, g, seed, opts):
    """The ends of the containment fixed points (second pass, the tail's two scans; fixed_point_kernels.hip): every list
    through the kernel for long lists (resident workgroups, a barrier per round; C5 takes it), a mix of both kernels,
    the host's loop of one look per round - and the long lists' kernel when its workgroups cannot meet (nothing
    guarantees that they are resident together): the last one to leave does the rounds alone.  "2": one
    workgroup stops waiting at every barrier behind the first, the last one included (passing and giving
    up are decided by one word - a barrier is passed by all or by none)."""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("n,g,seed", [(3000, 600_000, 21), (2000, 1_200_000, 33), (600, 60_000, 9)])
def test_host_tail_cross_check(hip_ctx_factory, n, g, seed):
    """use_gpu_tail = 0: Graph::preprocess on the host (the cross-check of the device tail)."""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_gpu_tail", 0)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


def _pinned_columns(ov):
    """the overlap columns in page-locked host memory (torch is plumbing here: pin_memory), as an object set_overlaps takes"""
    import torch
    from rala_amd.synth import FIELDS

    class _Cols:
        pass
    cols, keep = _Cols(), []
    for f in list(FIELDS) + ["strand"]:
        t = torch.from_numpy(np.ascontiguousarray(getattr(ov, f))).pin_memory()
        keep.append(t)
        setattr(cols, f, t.numpy())
    cols._keep = keep
    cols.__class__.__len__ = lambda self: len(ov)
    return cols


@pytest.mark.parametrize("side_stream,partitioned", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("n,g,seed", [(5000, 1_000_000, 7), (600, 60_000, 9)])
def test_columns_uploaded_inside_initialize(hip_ctx_factory, n, g, seed, side_stream, partitioned):
    """RALA_HIP_MEM_HOST_ASYNC: the host columns leave inside rala_hip_initialize, each in front of the first kernel that reads
    it (the partitioned bucketing with the counting pass's duplicate removal), or all of them in front of everything (the other
    paths); twice on one context, the second time over other data - what a failed or finished call left must not be read."""
    ds = Dataset(n, g, seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_side_stream", side_stream)
    ctx.set_option("use_partitioned_buckets", partitioned)
    other = Dataset(n, g, seed + 1)
    ctx.set_reads(other.read_len)
    ctx.set_overlaps(_pinned_columns(other.overlaps), later=True)
    ctx.initialize()
    ctx.set_reads(ds.read_len)
    for _ in range(2):
        ctx.set_overlaps(_pinned_columns(ds.overlaps), later=True)
        ctx.initialize()
        parity.check_initialize(ctx, st, ds)
        ctx.construct()
        parity.check_construct(ctx, st)
        parity.check_tr(ctx, st)


def test_columns_asked_for_before_initialize_has_uploaded_them(hip_ctx_factory):
    """RALA_HIP_MEM_HOST_ASYNC followed by a call that reads the columns first (rala_hip_dedupe, the getter): uploaded then"""
    ds = Dataset(3000, 600_000, 21)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(_pinned_columns(ds.overlaps), later=True)
    ctx.dedupe()
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)


@pytest.mark.parametrize("gpu_tail,run_kernel", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("n,g,seed", [(5000, 1_000_000, 7), (6000, 1_600_000, 19),
                                      (600, 60_000, 9),        # ~100x: beyond the 512-event tier
                                      (900, 30_000, 4)])       # ~300x: on to the position-space kernel
def test_sensitive_pass_vs_oracle(hip_ctx_factory, n, g, seed, gpu_tail, run_kernel):
    """Graph::preprocess(overlaps, sensitive path) (reference graph.cpp:882-1054), after the
    chimera stage on the device (default) or on the host; the second pass over the piles in run
    space (default: primary bound events + sensitive bounds, two tiers, the rest in position
    space) or all of it in position space."""
    _check_sensitive(hip_ctx_factory, Dataset(n, g, seed), gpu_tail, run_kernel, expect_hills=g >= 100_000)


@pytest.mark.parametrize("gpu_tail,run_kernel", [(1, 1), (0, 1), (1, 0)])
def test_sensitive_pass_with_pools_that_grow(hip_ctx_factory, gpu_tail, run_kernel):
    """both interval pools start at 16 slots (interval_pool_per_read_x1000 = 0): the first pass' pool and the repeat hills'
    pool are grown to the counted need, the stage / the pass' second mode runs again"""
    _check_sensitive(hip_ctx_factory, Dataset(6000, 1_600_000, 19), gpu_tail, run_kernel, expect_hills=True, small_pools=True)


@pytest.mark.parametrize("gpu_tail", [1, 0])
def test_sensitive_pass_with_lists_that_double(hip_ctx_factory, gpu_tail):
    """every read of the position-space kernels takes the way of the lists in global memory (debug_force_big), which start at
    four regions / four raw intervals (debug_big_caps): the repeat hills' second mode notes its reads and doubles the lists
    until they fit - pile_unbounded_reads grows inside construct"""
    _check_sensitive(hip_ctx_factory, Dataset(5000, 1_000_000, 7), gpu_tail, run_kernel=0, expect_hills=True,
                     options={"debug_force_big": 1, "debug_big_caps": (4 << 32) | 4}, lists_must_double=True)


@pytest.mark.parametrize("gpu_tail", [1, 0])
def test_sensitive_overlaps_in_device_memory(hip_ctx_factory, gpu_tail):
    """option sensitive_in_device_memory: the sensitive set handed to rala_hip_construct as device pointers (what
    bench.py's c3s / c5s workloads do: resident in HBM like the primary set)"""
    _check_sensitive(hip_ctx_factory, Dataset(5000, 1_000_000, 7), gpu_tail, 1, expect_hills=True, in_device=True)


def _check_sensitive(hip_ctx_factory, ds, gpu_tail, run_kernel, expect_hills, in_device=False, small_pools=False, options=None,
                     lists_must_double=False):
    from oracle.oracle import Oracle

    n = ds.n_reads
    o = Oracle(ds.read_len, ds.overlaps, n_threads=8)
    assert o.initialize() == 0
    o.pass2()
    o.preprocess_chimeras()
    p = o.piles()
    sens = ds.sensitive(p["alive"], p["begin"], p["end"])
    o.preprocess_repeats(sens)
    want_rep = o.all_intervals(2)
    want_flags = [o.repeat_flags(r) for r in range(n)]
    want_flags = np.concatenate(want_flags) if want_flags else np.zeros(0, np.uint8)
    want_ov = o.overlap_list(0)
    want_p = o.piles()
    o.build_graph()
    want_tr = o.remove_transitive_edges()
    want_e = o.edges()

    ctx = hip_ctx_factory()
    ctx.set_option("use_gpu_tail", gpu_tail)
    ctx.set_option("use_run_kernel", run_kernel)
    if small_pools:
        ctx.set_option("interval_pool_per_read_x1000", 0)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    unbounded_before = ctx.timings()["pile_unbounded_reads"]
    if in_device:
        from rala_amd import hip
        ctx.set_option("sensitive_in_device_memory", 1)
        dev = hip.DeviceOverlaps.from_host(sens, 0)
        ctx.construct(dev)
        ctx.initialize()                # (and again: the set is not consumed)
        ctx.construct(dev)
    else:
        ctx.construct(sens)
    if small_pools:
        assert len(want_rep[1]) > 16 and ctx.timings()["pool_regrown"] >= 1, (len(want_rep[1]), ctx.timings())
    if lists_must_double:
        assert ctx.timings()["pile_unbounded_reads"] > unbounded_before, (unbounded_before, ctx.timings())
    offs, pairs, flags = ctx.intervals(2)
    parity.assert_same("rep.offsets", offs, want_rep[0])
    parity.assert_same("rep.pairs", pairs, want_rep[1])
    parity.assert_same("rep.flags", flags.astype(np.uint8), want_flags)
    assert len(pairs) > 0 or not expect_hills, "the data set should exercise repeat hills"
    hp = ctx.piles()
    for k in ("alive", "begin", "end", "median", "p10"):
        parity.assert_same("piles." + k, hp[k], want_p[k])
    h = ctx.overlap_list(0)
    parity.assert_same("ov.src", h["src"], want_ov["src"].astype(np.uint32))
    assert ctx.remove_transitive_edges() == want_tr
    gr = ctx.graph()
    for k in ("src", "dst", "len", "marked"):
        parity.assert_same("edges." + k, gr[k], want_e[k])
    # coverage of a few targets after the second add_layers
    tg = np.unique(sens.b_id)[:16]
    for r in tg:
        parity.assert_same("pile_data[%d]" % r, ctx.pile_data(int(r)), o.pile_data(int(r)))


class _Scaled:
    """A synthetic data set with every coordinate and length multiplied by `factor`."""

    def __init__(self, ds, factor):
        from rala_amd.synth import Overlaps, FIELDS

        ov = ds.overlaps
        kw = {f: getattr(ov, f) for f in FIELDS}
        for f in ("a_begin", "a_end", "b_begin", "b_end", "length"):
            kw[f] = kw[f] * factor
        self.overlaps = Overlaps(strand=ov.strand, **kw)
        self.read_len = (ds.read_len * factor).astype(np.uint32)
        self.n_reads = ds.n_reads
        self.base, self.factor = ds, factor
        if hasattr(ds, "sensitive"):
            self.sensitive = self._sensitive

    def _sensitive(self, alive, begin, end):
        """sensitive overlaps of the base data set against its reads trimmed to [begin, end) / factor, scaled;
        target coordinates kept inside the trimmed target"""
        from rala_amd.synth import Overlaps, FIELDS

        f = self.factor
        begin, end = np.asarray(begin, dtype=np.uint32), np.asarray(end, dtype=np.uint32)
        sv = self.base.sensitive(alive, begin // f, end // f)
        kw = {k: np.array(getattr(sv, k), dtype=np.uint32) for k in FIELDS}
        for k in ("a_begin", "a_end", "b_begin", "b_end", "length"):
            kw[k] = kw[k] * f
        span = (end - begin)[kw["b_id"]]
        kw["b_end"] = np.minimum(kw["b_end"], span)
        keep = kw["b_begin"] + 200 < kw["b_end"]
        return Overlaps(strand=np.array(sv.strand, dtype=np.uint8)[keep], **{k: v[keep] for k, v in kw.items()})


@pytest.mark.parametrize("factor", [2, 3, 5, 7])
def test_long_reads(hip_ctx_factory, factor):
    """Reads longer than the first kernel's 16384-base bitmap (the length classes' own kernels:
    up to 32768, up to 65535), reads on both sides of 32768, and longer than 65536 bases (run
    starts beyond 16 bits: sorted-event path of the any-length kernel)."""
    ds = _Scaled(Dataset(1500, 300_000, 11), factor)
    assert ds.read_len.max() > {2: 16384, 3: 32768, 5: 32768, 7: 65536}[factor]
    if factor == 5:
        assert ((ds.read_len > 32768) & (ds.read_len <= 65535)).sum() > 1000
    if factor == 3:
        assert ((ds.read_len > 16384) & (ds.read_len <= 32768)).sum() > 100
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("side_stream", [1, 0])
@pytest.mark.parametrize("factor", [1, 2, 4])
def test_event_dense_reads_of_every_length_class(hip_ctx_factory, factor, side_stream):
    """~300x coverage: most reads have more events than the cap-512 kernels take and start in the cap-1024
    kernel from the list made of the bucket counts, some go on to cap 2048; with the longer length classes
    beside them on the same stream."""
    base = Dataset(1200, 40_000, 5)
    ds = _Scaled(base, factor) if factor > 1 else base
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_side_stream", side_stream)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    tm = ctx.timings()
    assert tm["pile_overflow_reads"] > 300, tm
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


@pytest.mark.parametrize("factor", [2, 3])
def test_sensitive_pass_long_reads(hip_ctx_factory, factor):
    """The second pass over the piles on reads beyond 16384 bases: its 32768-base kernel (factor 2), and
    the position-space kernel behind it for the still longer ones (factor 3)."""
    ds = _Scaled(Dataset(3000, 600_000, 7), factor)
    assert (ds.read_len > 16384).sum() > 2000
    _check_sensitive(hip_ctx_factory, ds, 1, 1, expect_hills=True)


def _shuffled_with_duplicates(ds, seed):
    """same data set, but every query's run of overlaps is shuffled and ~3 % of the records are
    repeated inside their run with other lengths (the general case of remove_duplicate_overlaps,
    reference graph.cpp:273-307), ~1 % of the target names do not resolve, a few self overlaps"""
    from rala_amd.synth import Overlaps, FIELDS

    rng = np.random.default_rng(seed)
    ov = ds.overlaps
    n = len(ov)
    dup = np.nonzero(rng.random(n) < 0.03)[0]
    idx = np.concatenate([np.arange(n), dup, dup[: len(dup) // 3]])
    run_key = ov.a_id[idx].astype(np.int64)
    order = np.lexsort((rng.random(len(idx)), run_key))          # group by query, random inside
    idx = idx[order]
    kw = {f: getattr(ov, f)[idx].copy() for f in FIELDS}
    strand = ov.strand[idx].copy()
    extra = np.arange(len(idx)) >= 0
    bump = rng.random(len(idx)) < 0.05
    kw["length"][bump] += rng.integers(0, 3, size=int(bump.sum())).astype(np.uint32)     # ties and near ties
    bad = rng.random(len(idx)) < 0.01
    kw["b_id"][bad] = 0xFFFFFFFF
    selfo = rng.random(len(idx)) < 0.002
    kw["b_id"][selfo] = kw["a_id"][selfo]
    kw["b_begin"][selfo] = kw["a_begin"][selfo]; kw["b_end"][selfo] = kw["a_end"][selfo]

    class _D:
        pass
    d = _D()
    d.overlaps = Overlaps(strand=strand, **kw)
    d.read_len = ds.read_len
    d.n_reads = ds.n_reads
    return d


@pytest.mark.parametrize("list_cap", [0, 5])
@pytest.mark.parametrize("n,g,seed", [(3000, 600_000, 21), (2000, 1_200_000, 33)])
def test_unordered_runs_duplicates_unresolved(hip_ctx_factory, n, g, seed, list_cap):
    """(runs shuffled inside: the counting pass's trips stage more marks than they hold and give the list up - a bit that
    stays set, advisor round 5; list_cap = 5: a list that overflows by its count)"""
    ds = _shuffled_with_duplicates(Dataset(n, g, seed), seed)
    st = parity.oracle_stages(ds)
    assert st["valid"].sum() < len(st["valid"])                  # duplicates were found
    ctx = hip_ctx_factory()
    ctx.set_option("debug_dedupe_list_cap", list_cap)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


def _few_duplicates(ds, seed):
    """the file as it is (grouped by query), one record in five hundred repeated right behind itself with another length: the
    counting pass marks a run here and there and lists the marks"""
    from rala_amd.synth import Overlaps, FIELDS

    rng = np.random.default_rng(seed)
    ov = ds.overlaps
    n = len(ov)
    dup = np.nonzero(rng.random(n) < 0.002)[0]
    idx = np.sort(np.concatenate([np.arange(n), dup]), kind="stable")
    kw = {f: getattr(ov, f)[idx].copy() for f in FIELDS}
    second = np.r_[False, idx[1:] == idx[:-1]]
    kw["length"][second] += rng.integers(0, 3, size=int(second.sum())).astype(np.uint32)

    class _D:
        pass
    d = _D()
    d.overlaps = Overlaps(strand=ov.strand[idx].copy(), **kw)
    d.read_len = ds.read_len
    d.n_reads = ds.n_reads
    return d


@pytest.mark.parametrize("list_cap", [0, 1, 7])
def test_few_duplicates_mark_list(hip_ctx_factory, list_cap):
    """duplicate removal inside the bucketing's counting pass: the marked runs redone from the list (list_cap 0 = 2^20 marks), and
    a list that does not hold its marks given up for the pass over all overlaps"""
    ds = _few_duplicates(Dataset(3000, 600_000, 21), 5)
    st = parity.oracle_stages(ds)
    assert 0 < len(st["valid"]) - st["valid"].sum() < len(st["valid"]) // 100
    ctx = hip_ctx_factory()
    ctx.set_option("debug_dedupe_list_cap", list_cap)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


def _queries_in_two_runs(ds, seed):
    """same overlaps, but one query in twelve has the second half of its run moved to the end of the file: a file that is NOT
    grouped by query (the reference takes runs as they come: duplicate removal per run, every bound into its pile)"""
    from rala_amd.synth import Overlaps, FIELDS

    rng = np.random.default_rng(seed)
    ov = ds.overlaps
    a = ov.a_id.astype(np.int64)
    n = len(a)
    start = np.r_[0, np.nonzero(a[1:] != a[:-1])[0] + 1]
    end = np.r_[start[1:], n]
    moved = np.zeros(n, dtype=bool)
    for s0, e0 in zip(start, end):
        if e0 - s0 >= 4 and rng.random() < 1.0 / 12:
            moved[(s0 + e0) // 2:e0] = True
    idx = np.r_[np.nonzero(~moved)[0], np.nonzero(moved)[0]]
    assert moved.sum() > 0

    class _D:
        pass
    d = _D()
    d.overlaps = Overlaps(strand=ov.strand[idx].copy(), **{f: getattr(ov, f)[idx].copy() for f in FIELDS})
    d.read_len = ds.read_len
    d.n_reads = ds.n_reads
    return d


@pytest.mark.parametrize("partitioned", [1, 0])
@pytest.mark.parametrize("n,g,seed", [(3000, 600_000, 21), (600, 60_000, 9)])
def test_queries_in_two_runs(hip_ctx_factory, n, g, seed, partitioned):
    """a file that is not grouped by query: the bucketing's last kernel may not copy a read's query side from its run of the
    file (there are two), the pass over all overlaps writes it (and the other bucketing path never looked at runs)"""
    ds = _queries_in_two_runs(Dataset(n, g, seed), seed)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_partitioned_buckets", partitioned)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


def test_degenerate_inputs(hip_ctx_factory):
    from rala_amd import hip
    from rala_amd.synth import Overlaps, FIELDS

    # no overlaps at all: every read is filtered ("filtered all sequences", graph.cpp:418-421)
    ctx = hip_ctx_factory()
    ctx.set_reads(np.array([5000, 7000, 9000], dtype=np.uint32))
    empty = Overlaps(strand=np.zeros(0, np.uint8), **{f: np.zeros(0, np.uint32) for f in FIELDS})
    ctx.set_overlaps(empty)
    with pytest.raises(hip.RalaHipError) as e:
        ctx.initialize()
    assert e.value.code == -4
    # one read, overlaps that only name unknown reads
    ctx = hip_ctx_factory()
    ctx.set_reads(np.array([8000], dtype=np.uint32))
    kw = {f: np.array([0xFFFFFFFF, 0], dtype=np.uint32) if f in ("a_id", "b_id") else np.array([100, 100], dtype=np.uint32)
          for f in FIELDS}
    kw["a_end"] = kw["b_end"] = np.array([4000, 4000], dtype=np.uint32)
    kw["length"] = np.array([3900, 3900], dtype=np.uint32)
    kw["b_id"] = np.array([0, 0xFFFFFFFF], dtype=np.uint32)
    ctx.set_overlaps(Overlaps(strand=np.zeros(2, np.uint8), **kw))
    with pytest.raises(hip.RalaHipError) as e:
        ctx.initialize()
    assert e.value.code == -4
    assert ctx.valid().tolist() == [0, 0]


@pytest.mark.parametrize("run_kernel,n,g,seed,factor", [(0, 1500, 300_000, 11, 1), (0, 1500, 300_000, 11, 7),
                                                       (1, 1500, 12_000, 3, 1)])
def test_position_kernel_slab_path(hip_ctx_factory, run_kernel, n, g, seed, factor):
    """max_lds_read_len = 0: the position-space kernel keeps its three per-read arrays in HBM
    slabs instead of LDS (what it does for reads too long for LDS) - every read with
    use_run_kernel = 0, the reads beyond the 2048-event cap otherwise."""
    ds = Dataset(n, g, seed)
    if factor > 1:
        ds = _Scaled(ds, factor)
    st = parity.oracle_stages(ds)
    ctx = hip_ctx_factory()
    ctx.set_option("use_run_kernel", run_kernel)
    ctx.set_option("max_lds_read_len", 0)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    if run_kernel:
        assert ctx.timings()["pile_position_reads"] > 0


def test_interval_pool_grows_to_the_counted_need(hip_ctx_factory):
    """a pit / hill pool that turns out too small (interval_pool_per_read_x1000 is a hint) is grown to what the kernels
    counted and the stage runs again - the reference's lists are vectors (pile.hpp:164-169); round 3 returned
    RALA_HIP_ECAPACITY here"""
    ds = Dataset(40_000, 8_000_000, 13)
    st = parity.oracle_stages(ds)
    n_iv = len(st["pits0"][1]) + len(st["hills0"][1])
    assert n_iv > 1024, "the data set should need more than the floor of the pool"
    ctx = hip_ctx_factory()
    ctx.set_option("interval_pool_per_read_x1000", 1)          # 1024 slots (the floor) for 40 k reads
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)
    ctx.initialize()
    assert ctx.timings()["pool_regrown"] == 1
    parity.check_initialize(ctx, st, ds)
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)
    ctx.initialize()                                           # the pool keeps its size
    assert ctx.timings()["pool_regrown"] == 0
    parity.check_initialize(ctx, st, ds)


def test_device_resident_overlaps_and_prefilter_count(hip_ctx_factory):
    """rala_hip_set_overlaps(RALA_HIP_MEM_DEVICE): the columns are adopted where they lie in HBM
    (here torch tensors); num_prefiltered is the reference's "prefiltered sequences" count."""
    import torch
    from rala_amd.synth import FIELDS

    ds = Dataset(3000, 600_000, 21)
    st = parity.oracle_stages(ds)
    o = st["oracle"]
    cols = {f: torch.from_numpy(np.ascontiguousarray(getattr(ds.overlaps, f)).astype(np.int64)).to(torch.int32).cuda()
            for f in FIELDS}
    cols["strand"] = torch.from_numpy(np.ascontiguousarray(ds.overlaps.strand)).cuda()
    torch.cuda.synchronize()
    ctx = hip_ctx_factory()
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps_device({k: v.data_ptr() for k, v in cols.items()}, len(ds.overlaps))
    ctx.initialize()
    parity.check_initialize(ctx, st, ds)
    assert ctx.num_prefiltered() == int(o.L.ora_n_prefiltered(o.h))
    assert ctx.num_prefiltered() == int((st["piles0"]["alive"] == 0).sum())
    ctx.construct()
    parity.check_construct(ctx, st)
    parity.check_tr(ctx, st)


def test_call_order_and_argument_errors(hip_ctx_factory):
    """the C ABI refuses calls out of order the way the reference does ("object already
    constructed", graph.cpp:431-435) and reports bad arguments instead of acting on them"""
    from rala_amd import hip

    def code(fn, *a):
        with pytest.raises(hip.RalaHipError) as e:
            fn(*a)
        return e.value.code

    ds = Dataset(1000, 200_000, 1)
    ctx = hip_ctx_factory()
    assert code(ctx.initialize) == -2                      # no reads set
    assert code(ctx.set_option, "no_such_option", 1) == -2
    ctx.set_reads(ds.read_len)
    assert code(ctx.initialize) == -2                      # neither overlaps nor bound tuples set
    assert code(ctx.dedupe) == -2
    ctx.set_overlaps(ds.overlaps)
    assert code(ctx.construct) == -2                       # initialize first
    assert code(ctx.piles) == -2
    assert code(ctx.intervals, 0) == -2
    ctx.initialize()
    assert code(ctx.intervals, 3) == -2                    # no such kind
    buf = np.zeros(16, dtype=np.uint16)
    assert ctx.L.rala_hip_get_pile_data(ctx.h, ds.n_reads, buf.ctypes.data) == -2      # read out of range
    assert code(ctx.remove_transitive_edges) == -2         # construct first
    assert code(ctx.graph) == -2
    assert code(ctx.overlap_list, 0) == -2
    ctx.construct()
    assert code(ctx.construct) == -2                       # already constructed
    n = ctx.remove_transitive_edges()
    # a second initialize starts over on the same context
    ctx.initialize()
    ctx.construct()
    assert ctx.remove_transitive_edges() == n


def test_inputs_in_either_order_and_context_reuse(hip_ctx_factory):
    """overlaps before reads, and a context used again with MORE reads than overlaps (the scan
    workspace has to follow the larger of the two whichever call comes last)"""
    from oracle.oracle import Oracle

    ds = Dataset(1500, 300_000, 9)
    o = Oracle(ds.read_len, ds.overlaps, n_threads=4)
    o.construct()
    ctx = hip_ctx_factory()
    ctx.set_reads(ds.read_len[:10])
    ctx.set_overlaps(ds.overlaps.take(slice(0, 0)))
    # now the real inputs, reads last
    ctx.set_overlaps(ds.overlaps)
    ctx.set_reads(ds.read_len)
    ctx.initialize()
    ctx.construct()
    want, got = o.piles(), ctx.piles()
    for k in ("alive", "begin", "end", "median"):
        assert (got[k] == want[k]).all(), k
    # many reads, few overlaps (n_reads > n_overlaps)
    few = ds.overlaps.take(slice(0, 50))
    big_len = np.concatenate([ds.read_len] * 4)
    ctx.set_overlaps(few)
    ctx.set_reads(big_len)
    try:
        ctx.initialize()
    except Exception as e:          # everything filtered is a legitimate outcome here
        assert getattr(e, "code", 0) == -4
