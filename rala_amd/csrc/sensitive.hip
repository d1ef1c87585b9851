// librala_hip: Graph::preprocess with the sensitive overlaps - the two modes of the sensitive pass over the piles, the repeat
// hills, the overlaps they rule out.  Implements rala_hip_find_repetitive_hills of rala_hip.h and repeats_stage of stages.h;
// rala_hip_construct's cross-check path calls preprocess_repeats (orchestration.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "lifecycle.h"
#include "orchestration.h"

using namespace rala_hip;

namespace {

// position-space sensitive-pass kernel over `reads`, grouped by LDS image size, on stream st (the main stream, or the aux
// stream beside a mode's run-space kernels: nothing here waits for another stream).  Mode 2, a.big_cap_reg != 0: with the
// region lists and raw hills in global memory at those sizes.
int run_repeats_classes_on_rows(rala_hip_ctx* ctx, const RepeatArgs& a, const std::vector<uint32_t>& reads, int mode, hipStream_t st) {
    return launch_by_class(ctx, a, reads, mode == 2 && a.big_cap_reg != 0, repeats_big_words, st, "repeats",
                           [&](const RepeatArgs& c, uint32_t grid, bool in_lds) { launch_pile_repeats(c, grid, in_lds, mode, st); });
}

// position-space sensitive-pass kernel over `reads` where the rows are: the resident ones, or - option pile_rows = 0 - batch
// after batch of them rebuilt in the scratch, a.pile / a.pile_off pointing there (mode 1 works on top of the primary rows; mode
// 2 reads them with the sensitive layers of this construct on top, as the resident rows hold them by then)
int run_repeats_classes(rala_hip_ctx* ctx, RepeatArgs a, const std::vector<uint32_t>& reads, int mode, hipStream_t st) {
    if (!ctx->rowless) return run_repeats_classes_on_rows(ctx, a, reads, mode, st);
    const uint64_t cap = rows_scratch_cap(ctx);
    for (size_t i = 0; i < reads.size();) {
        size_t j = i;
        uint64_t total = 0;
        do total += scratch_row_elems(ctx->h_read_len[reads[j++]]);
        while (j < reads.size() && total + scratch_row_elems(ctx->h_read_len[reads[j]]) <= cap);
        const std::vector<uint32_t> part(reads.begin() + i, reads.begin() + j);
        int rc = materialize_rows(ctx, part.data(), 0, (uint32_t)part.size(), mode == 2 && (ctx->sens_csr_ready || ctx->sens_pass_running), st);
        if (rc != RALA_HIP_OK) return rc;
        a.pile = ctx->d_rows_scratch.p; a.pile_off = ctx->d_rows_off.p;
        rc = run_repeats_classes_on_rows(ctx, a, part, mode, st);
        if (rc != RALA_HIP_OK) return rc;
        i = j;
    }
    return RALA_HIP_OK;
}

// The repeat-hill kernel in position space over `reads`, on stream st (null: the main stream).  Mode 2: a read whose region
// lists or raw hills outgrow the kernel's LDS lists is noted and runs again with the lists in global memory
// (run_until_lists_fit, as the pile kernel's noted reads).
int run_repeats_kernel(rala_hip_ctx* ctx, RepeatArgs a, const std::vector<uint32_t>& reads, int mode, hipStream_t st = nullptr) {
    if (reads.empty()) return RALA_HIP_OK;
    if (st == nullptr) st = ctx->stream;
    if (mode != 2) return run_repeats_classes(ctx, a, reads, mode, st);
    uint32_t* const count_dev = ctx->d_small.p + kSensNotedReads;
    HIPCHECK(ctx->d_big_list[0].ensure(ctx->n_reads + 1));
    HIPCHECK(hipMemsetAsync(count_dev, 0, 4, st));
    a.big_list = ctx->d_big_list[0].p;
    a.big_count = count_dev;
    a.big_space = nullptr; a.big_cap_reg = a.big_cap_list = a.big_cap_raw = 0;
    a.force_big = ctx->debug_force_big ? 1u : 0u;
    const int rc = run_repeats_classes(ctx, a, reads, 2, st);
    if (rc != RALA_HIP_OK) return rc;
    // one look: the status word and how many reads were noted (a copy on THIS stream - a blocking copy would wait for the
    // run-space kernels beside)
    uint32_t look[kSensLookWords] = {};
    HIPCHECK(hipMemcpyAsync(look, ctx->d_small.p + kSensStatus, sizeof(look), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    const uint32_t count = look[kSensNotedReads - kSensStatus];
    if (count == 0) return RALA_HIP_OK;
    ctx->tm.pile_unbounded_reads += count;
    return run_until_lists_fit(ctx, count, count_dev, ctx->d_small.p + kSensStatus, 2, st, "repeat hills, ",
                               "repeat-hill kernel: reads left without a reason",
                               [&](const std::vector<uint32_t>& again, uint32_t* note_in, uint32_t cap_reg, uint32_t cap_list, uint32_t cap_raw) {
                                   a.big_list = note_in;
                                   a.big_cap_reg = cap_reg; a.big_cap_list = cap_list; a.big_cap_raw = cap_raw;
                                   return run_repeats_classes(ctx, a, again, 2, st);
                               });
}

// One mode of the sensitive pass over the reads of a device list (its length in *count_dev, at most `bound`): every read
// starts in the kernel that fits it, known beforehand from its length and its primary + sensitive event count
// (launch_sens_split) - cap 512 / 16384 bases and cap 512 / 32768 bases on the main stream; cap 1024 / 16384 bases and, behind
// it, the position-space kernel for what fits neither (the event-dense reads: 6 842 of C5's 281 k targets, a third of the
// pass when they ran behind the others) BESIDE them on the aux stream (round 5).  What a kernel still hands on (its region
// lists) goes down the chain behind the join: cap 512 -> cap 1024 -> position space; usually nothing.
// Two looks from the host: the classes' sizes (with whatever the caller has queued on this context: d2h_small), and the
// hand-over counts at the end - which come with the sixteen words of d_small (the repeat hills' pool counter and the status
// word among them) in `small16`.  *count_out: the list's length.
int run_sens_pass(rala_hip_ctx* ctx, PileArgs pa, const RepeatArgs& ra, int mode, const uint32_t* list_dev, uint32_t bound,
                  const uint32_t* count_dev, uint32_t* count_out, uint32_t* small16) {
    *count_out = 0;
    if (bound == 0) return RALA_HIP_OK;
    hipStream_t s = ctx->stream;
    Trace trc;
    if (!ctx->use_run_kernel || !ctx->ev_ready) {
        uint32_t count = 0;
        HIPCHECK(d2h_small(ctx, &count, count_dev, 4, s));
        HIPCHECK(stream_sync(ctx, s));
        *count_out = count;
        std::vector<uint32_t> host(count);
        if (count) HIPCHECK(hipMemcpy(host.data(), list_dev, (size_t)count * 4, hipMemcpyDeviceToHost));
        std::sort(host.begin(), host.end());
        const int rc = run_repeats_kernel(ctx, ra, host, mode);
        if (rc != RALA_HIP_OK) return rc;
        HIPCHECK(hipMemcpy(small16, ctx->d_small.p, kSmallWords * 4, hipMemcpyDeviceToHost));
        return RALA_HIP_OK;
    }
    HIPCHECK(ctx->d_overflow.ensure(ctx->n_reads + 1));
    HIPCHECK(ctx->d_overflow_mid.ensure(ctx->n_reads + 1));
    HIPCHECK(ctx->d_chain_cnt.ensure(kChainWords));
    // (what the cap-512 kernels hand on, what the cap-1024 and cap-2048 kernels hand on, the classes' sizes: slots.h)
    uint32_t* const from_512 = ctx->d_chain_cnt.p + kChainFrom512;
    uint32_t* const from_1024 = ctx->d_chain_cnt.p + kChainFrom1024;
    {
        FillList fills;
        fills.add(from_512, 0, kChainHandedWords * 4);
        fills.add(ctx->d_chain_cnt.p + kChainClasses, 0, kChainClassWords * 4);
        HIPCHECK(fills.launch(s));
    }
    HIPCHECK(ctx->d_sens_split.ensure(kChainClassWords * ((size_t)bound + 1)));
    SensSplitArgs sp;
    sp.read_len = pa.read_len; sp.ev_off = pa.ev_off; sp.ev_cnt = pa.ev_cnt; sp.ev_stride = pa.ev_stride; sp.ev_shift = pa.ev_shift;
    sp.sens_off = pa.sens_off; sp.begin = pa.begin; sp.end = pa.end;
    for (uint32_t c = 0; c < kChainClassWords; ++c) sp.out[c] = ctx->d_sens_split.p + (size_t)c * ((size_t)bound + 1);
    sp.counts = ctx->d_chain_cnt.p + kChainClasses;
    launch_sens_split(list_dev, bound, count_dev, sp, s);
    // look 1: the classes' sizes, the list's length; the first reads of the position-space class ride along
    constexpr uint32_t kRestAhead = 16384;
    HIPCHECK(ctx->p_sens_rest.ensure(kRestAhead));
    uint32_t cls[kChainClassWords] = {}, count = 0;
    HIPCHECK(d2h_small(ctx, cls, ctx->d_chain_cnt.p + kChainClasses, sizeof(cls), s));
    HIPCHECK(d2h_small(ctx, &count, count_dev, 4, s));
    HIPCHECK(hipMemcpyAsync(ctx->p_sens_rest.p, sp.out[kClassPosition], (size_t)std::min<uint32_t>(bound, kRestAhead) * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    *count_out = count;
    if (count == 0) {
        HIPCHECK(hipMemcpy(small16, ctx->d_small.p, kSmallWords * 4, hipMemcpyDeviceToHost));
        return RALA_HIP_OK;
    }
    uint32_t* const handed_512 = ctx->d_overflow.p;            // -> cap 1024
    uint32_t* const handed_1024 = ctx->d_overflow_mid.p;       // -> position space
    // (three streams: the two cap-512 kernels on the main one, the cap-1024 kernel on aux, the position-space kernels - whose
    // host side waits for its own stream between its steps - on side.  First version of this round: both of the latter on aux,
    // and the wait for the rest of a long class-3 list was a wait for the cap-1024 kernel: C5 12.4 ms, no gain)
    hipStream_t aux = ctx->use_side_stream ? ctx->aux : s;
    hipStream_t pos = ctx->use_side_stream ? ctx->side : s;
    if (aux != s) {
        HIPCHECK(hipEventRecord(ctx->ev[kEvSensFork], s));
        HIPCHECK(hipStreamWaitEvent(aux, ctx->ev[kEvSensFork], 0));
        HIPCHECK(hipStreamWaitEvent(pos, ctx->ev[kEvSensFork], 0));
    }
    pa.n_items_dev = nullptr;
    pa.order = sp.out[kClassCap512]; pa.n_items = cls[kClassCap512];
    launch_pile_sens(pa, cls[kClassCap512], PileTier::kCap512First, mode, handed_512, from_512, s);
    pa.order = sp.out[kClassCap512Long]; pa.n_items = cls[kClassCap512Long];
    launch_pile_sens(pa, std::min<uint32_t>(cls[kClassCap512Long], 16384), PileTier::kUpTo32k, mode, handed_512, from_512, s);
    pa.order = sp.out[kClassCap1024]; pa.n_items = cls[kClassCap1024];
    launch_pile_sens(pa, std::min<uint32_t>(cls[kClassCap1024], 8192), PileTier::kCap1024, mode, handed_1024, from_1024, aux);
    if (aux != s) HIPCHECK(hipEventRecord(ctx->ev[kEvSensAuxDone], aux));
    // (the event-dense reads: run space at 2048 events, one wavefront per SIMD - 6 842 of C5's 281 k targets took as long in
    // position space as all the others in theirs; what this kernel hands on goes down the chain with the cap-1024 kernel's)
    pa.order = sp.out[kClassCap2048]; pa.n_items = cls[kClassCap2048];
    launch_pile_sens(pa, std::min<uint32_t>(cls[kClassCap2048], 4096), PileTier::kCap2048, mode, handed_1024, from_1024, pos);
    if (const uint32_t n_rest = cls[kClassPosition]) {
        std::vector<uint32_t> rest(ctx->p_sens_rest.p, ctx->p_sens_rest.p + std::min<uint32_t>(n_rest, kRestAhead));
        if (n_rest > kRestAhead) {
            rest.resize(n_rest);
            HIPCHECK(hipMemcpyAsync(rest.data() + kRestAhead, sp.out[kClassPosition] + kRestAhead, (size_t)(n_rest - kRestAhead) * 4, hipMemcpyDeviceToHost, pos));
            HIPCHECK(hipStreamSynchronize(pos));
        }
        std::sort(rest.begin(), rest.end());
        const int rc = run_repeats_kernel(ctx, ra, rest, mode, pos);
        if (rc != RALA_HIP_OK) return rc;
        trc("sens pass: position space beside", rest.size());
    }
    if (aux != s) {
        HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvSensAuxDone], 0));
        if (cls[kClassCap2048] || cls[kClassPosition]) {
            HIPCHECK(hipEventRecord(ctx->ev[kEvSensPosDone], pos));
            HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvSensPosDone], 0));
        }
    }
    pa.order = handed_512; pa.n_items = count; pa.n_items_dev = from_512;
    launch_pile_sens(pa, std::min<uint32_t>(count, 2048), PileTier::kCap1024, mode, handed_1024, from_1024, s);
    // look 2: what was handed on, and the call's counters
    uint32_t handed[kChainLookWords] = {};
    HIPCHECK(d2h_small(ctx, handed, from_512, sizeof(handed), s));
    HIPCHECK(d2h_small(ctx, small16, ctx->d_small.p, kSmallWords * 4, s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    trc(mode == 1 ? "sens pass 1: run space" : "sens pass 2: run space", count);
    if (trace_on()) {
        fprintf(stderr, "[trace] sens pass %d: classes %u / %u / %u / %u / %u, handed on %u + %u\n", mode, cls[kClassCap512], cls[kClassCap512Long], cls[kClassCap1024],
                cls[kClassCap2048], cls[kClassPosition], handed[kChainFrom512], handed[kChainFrom1024]);
    }
    const uint32_t n_rest = handed[kChainFrom1024];
    if (n_rest == 0) return RALA_HIP_OK;
    std::vector<uint32_t> rest((size_t)n_rest);
    HIPCHECK(hipMemcpy(rest.data(), handed_1024, (size_t)n_rest * 4, hipMemcpyDeviceToHost));
    std::sort(rest.begin(), rest.end());
    const int rc = run_repeats_kernel(ctx, ra, rest, mode);
    trc("sens pass: position space", rest.size());
    if (rc != RALA_HIP_OK) return rc;
    HIPCHECK(hipMemcpy(small16, ctx->d_small.p, kSmallWords * 4, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

// Pile::is_valid_overlap (pile.cpp:605-630)
bool is_valid_overlap(rala_hip_ctx* ctx, uint32_t r, uint32_t x, uint32_t y) {
    const uint32_t B = ctx->h_begin[r], E = ctx->h_end[r];
    const Interval* h = ctx->h_rep_pool.data() + (ctx->h_n_rep[r] ? ctx->h_rep_slot[r] : 0);
    for (uint32_t i = 0; i < ctx->h_n_rep[r]; ++i) {
        if (!(x < h[i].second && h[i].first < y)) continue;
        if ((double)h[i].first < 0.1 * (double)(E - B) + (double)B) {
            if (y < h[i].second + kHillFuzz && h[i].aux) return false;
        } else if ((double)h[i].second > 0.9 * (double)(E - B) + (double)B) {
            if (x + kHillFuzz > h[i].first && h[i].aux) return false;
        }
    }
    return true;
}

// the sensitive pass behind the device-resident chimera stage (gpu_tail_part_a): repeats, final
// filter, then the final list and the graph (gpu_tail_part_b) - nothing comes to the host
int repeats_after_tail(rala_hip_ctx* cs, rala_hip_ctx* cl, Comm* comm, const rala_hip_overlaps* sens, uint64_t n_sens) {
    rala_hip_ctx* ctx = cs;
    hipStream_t s = cs->stream;
    Trace trs;
    launch_finalize_states(tail_list(cs), cs->d_alive.p, s);
    const int rc3 = preprocess_repeats(cs, cl, comm, sens, n_sens, true);
    if (rc3 != RALA_HIP_OK) return rc3;
    trs("sens: preprocess_repeats");
    const int rc4 = gpu_tail_part_b(cs);
    if (rc4 != RALA_HIP_OK) return rc4;
    trs("sens: final list + graph");
    HIPCHECK(stream_sync(cs, s));
    return RALA_HIP_OK;
}

}  // namespace

// the repeat hills (sensitive pass) as the host getters want them
int rala_hip::download_repeat_hills(rala_hip_ctx* ctx) {
    if (!ctx->rep_host_stale) return RALA_HIP_OK;
    const uint64_t n = ctx->n_reads;
    HIPCHECK(hipSetDevice(ctx->device));
    ctx->h_n_rep.resize(n); ctx->h_rep_slot.resize(n);
    HIPCHECK(hipMemcpy(ctx->h_n_rep.data(), ctx->d_n_rep.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(ctx->h_rep_slot.data(), ctx->d_rep_slot.p, n * 4, hipMemcpyDeviceToHost));
    ctx->h_rep_pool.resize(ctx->n_rep_hills);
    if (ctx->n_rep_hills) {
        HIPCHECK(hipMemcpy(ctx->h_rep_pool.data(), ctx->d_rep_pool.p, (size_t)ctx->n_rep_hills * sizeof(Interval), hipMemcpyDeviceToHost));
    }
    repeat_hills_fetched(ctx);
    return RALA_HIP_OK;
}

// Graph::preprocess(overlaps, sensitive path) (graph.cpp:882-1054).  Sensitive records:
// a = query (original read, untrimmed coordinates), b = target (trimmed read of the -p run).
//
// cs holds all reads and the lists the chimera stage left (on the host); cl holds the piles.  On
// one GPU they are the same context and comm is null.  In a sharded run cs holds this rank's
// share of the sensitive overlaps and cl the reads this rank owns (local read j = read j * P +
// rank): the target bounds travel to the owners in ONE all-to-all, the owners add the layers,
// take the medians and - once the component medians are known everywhere - look for the repeat
// hills; medians and hills are all-gathered, the hills' bridged flags all-reduced (max).
int rala_hip::preprocess_repeats(rala_hip_ctx* cs, rala_hip_ctx* cl, Comm* comm, const rala_hip_overlaps* sens, uint64_t n_sens,
                       bool device_lists) {
    // device_lists: the chimera stage left its lists, valid regions and liveness on the device
    // (gpu_tail_part_a); components, the final filter and (afterwards) the graph stay there too
    rala_hip_ctx* ctx = cs;                               // error reporting (HIPCHECK / fail)
    const bool sharded = comm != nullptr;
    const uint32_t P = sharded ? comm->world() : 1u, me = sharded ? comm->rank() : 0u;
    const uint64_t n = cs->n_reads;                       // all reads
    const uint64_t nl = cl->n_reads;                      // the reads whose piles are here
    const uint64_t nl_pad = ((n + P - 1) / P + 15) / 16 * 16;
    hipStream_t s = cs->stream;
    hipStream_t sl = cl->stream;
    Trace trc;
    auto comm_fail = [&](const char* what) {
        cs->err = std::string(what) + ": " + comm->error();
        cs->stage_pending.clear();
        cs->stage_used = 0;
        return RALA_HIP_EDEVICE;
    };
    if (n_sens >= 0x7FFFFFF0ull / 2) return fail(ctx, RALA_HIP_EINVAL, "too many sensitive overlaps");
    // the sensitive overlaps stay on the device from here on: columns as given (uploaded, or
    // adopted when the caller says they are device memory)
    OvlSoA so;
    {
        const uint32_t* src[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        const uint8_t* dev_strand = nullptr;
        if (n_sens) {
            src[0] = sens->a_id; src[1] = sens->b_id; src[2] = sens->a_begin; src[3] = sens->a_end;
            src[4] = sens->b_begin; src[5] = sens->b_end; src[6] = sens->length;
            dev_strand = sens->strand;
        }
        const uint32_t* dev[7];
        for (int k = 0; k < 7; ++k) dev[k] = src[k];
        if (!cs->sens_in_device) {
            for (int k = 0; k < 7; ++k) {
                HIPCHECK(cs->d_sens_col[k].ensure(n_sens));
                if (n_sens) HIPCHECK(hipMemcpyAsync(cs->d_sens_col[k].p, src[k], n_sens * 4, hipMemcpyHostToDevice, s));
                dev[k] = cs->d_sens_col[k].p;
            }
            HIPCHECK(cs->d_sens_strand.ensure(n_sens));
            if (n_sens) HIPCHECK(hipMemcpyAsync(cs->d_sens_strand.p, sens->strand, n_sens, hipMemcpyHostToDevice, s));
            dev_strand = cs->d_sens_strand.p;
        }
        so.a_id = dev[0]; so.b_id = dev[1]; so.a_begin = dev[2]; so.a_end = dev[3];
        so.b_begin = dev[4]; so.b_end = dev[5]; so.length = dev[6]; so.strand = dev_strand; so.n = n_sens; so.base = 0;
    }
    if (!device_lists) {
        // current valid regions and liveness on the device (a host tail narrowed them on the host)
        HIPCHECK(hipMemcpyAsync(cs->d_begin.p, cs->h_begin.data(), n * 4, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(cs->d_end.p, cs->h_end.data(), n * 4, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(cs->d_alive.p, cs->h_alive.data(), n, hipMemcpyHostToDevice, s));
    }
    // Overlap::transmute_ (overlap.cpp:84-114) + bounds of the targets, no +-15 (graph.cpp:929-933)
    for (int k = 0; k < 2; ++k) HIPCHECK(cs->d_sens_tb[k].ensure(n_sens));
    HIPCHECK(cs->d_sens_tuples.ensure(2 * n_sens + 8));
    HIPCHECK(cs->d_dataset_median.ensure(n));
    HIPCHECK(cs->d_n_rep.ensure(n));
    HIPCHECK(cs->d_rep_slot.ensure(n));
    cs->rep_pool_cap = std::max(cs->rep_pool_cap, cs->pool_cap_first);
    HIPCHECK(cs->d_rep_pool.ensure(cs->rep_pool_cap));
    HIPCHECK(hipMemsetAsync(cs->d_n_rep.p, 0, n * 4, s));
    HIPCHECK(hipMemsetAsync(cs->d_small.p + kSensPoolCount, 0, kSensPoolWords * 4, s));
    HIPCHECK(hipMemsetAsync(cs->d_small.p + kSensBadRecord, 0, 4, s));
    // One context: the target bounds as ONE 8-byte record per overlap, bucketed by the partitioned path the owners' records
    // of a sharded run take (bucket_kernels.hip; no +-15 here) - where the set suits that path; two tuples per overlap through
    // count / scan / scatter otherwise (and in a sharded run, where the tuples travel first)
    const BucketTuning bt = {cl->debug_part_shift, cl->debug_count_window};
    const bool sens_records = !sharded && cl->use_partitioned_buckets && n < (1u << kBoundRecordReadBits) - 1u &&
                              partition_path_fits_records((uint32_t)nl, cl->max_read_len, 2 * n_sens, bt);
    if (sens_records) {
        HIPCHECK(cs->d_sens_rec.ensure(n_sens + 8));
        launch_sens_records(so, (uint32_t)n, cs->d_begin.p, cs->d_alive.p, cs->d_sens_tb[0].p, cs->d_sens_tb[1].p, cs->d_sens_rec.p,
                            cs->d_small.p + kSensBadRecord, s);
    } else {
        launch_sens_tuples(so, (uint32_t)n, cs->d_begin.p, cs->d_alive.p, cs->d_sens_tb[0].p, cs->d_sens_tb[1].p,
                           cs->d_sens_tuples.p, cs->d_small.p + kSensBadRecord, s);
    }
    const uint2* tuples = cs->d_sens_tuples.p;          // what the pile holder buckets: {its read, bound}
    uint64_t n_tuples = 2 * n_sens;
    if (sharded) {
        // by owner of the target, ONE all-to-all
        HIPCHECK(cs->d_owner_cnt.ensure(2 * 64));
        HIPCHECK(cs->d_sens_part.ensure(2 * n_sens + 8));
        uint32_t* cnt = cs->d_owner_cnt.p;
        uint32_t* cur = cnt + 64;
        HIPCHECK(hipMemsetAsync(cnt, 0, 2 * 64 * 4, s));
        launch_partition_tuples(cs->d_sens_tuples.p, 2 * n_sens, P, 0, cnt, cs->d_sens_part.p, s);
        uint32_t h[64];
        HIPCHECK(hipMemcpyAsync(h, cnt, P * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(stream_sync(cs, s));
        uint32_t off[64];
        std::vector<uint64_t> send_counts(P), matrix((size_t)P * P), recv_counts(P);
        uint32_t acc = 0;
        for (uint32_t p = 0; p < P; ++p) { off[p] = acc; acc += h[p]; send_counts[p] = h[p]; }
        HIPCHECK(hipMemcpyAsync(cur, off, P * 4, hipMemcpyHostToDevice, s));
        launch_partition_tuples(cs->d_sens_tuples.p, 2 * n_sens, P, 1, cur, cs->d_sens_part.p, s);
        // a bad record anywhere is everybody's error
        if (comm->all_reduce_u32(cs->d_small.p + kSensBadRecord, 1, ReduceOp::kMax, s) != 0) return comm_fail("all-reduce of the record check");
        if (comm->host_all_gather(send_counts.data(), P, matrix.data(), s) != 0) return comm_fail("sensitive tuple counts");
        n_tuples = 0;
        for (uint32_t p = 0; p < P; ++p) { recv_counts[p] = matrix[(size_t)p * P + me]; n_tuples += recv_counts[p]; }
        HIPCHECK(cs->d_sens_recv.ensure(n_tuples + 8));
        if (comm->all_to_all_v(cs->d_sens_part.p, send_counts.data(), cs->d_sens_recv.p, recv_counts.data(), sizeof(uint2), s) != 0) {
            return comm_fail("all-to-all of the sensitive bounds");
        }
        tuples = cs->d_sens_recv.p;
        // the owner's copy of the current valid regions (the chimera stage narrowed them everywhere)
        HIPCHECK(stream_sync(cs, s));
        launch_localize_u32(cs->d_begin.p, nl, P, me, cl->d_begin.p, sl);
        launch_localize_u32(cs->d_end.p, nl, P, me, cl->d_end.p, sl);
        launch_localize_u8(cs->d_alive.p, nl, P, me, cl->d_alive.p, sl);
    }
    // (one context: the record check comes back with the first look of the pass below - a record that is an error names no
    // read, nothing downstream trips over it; a sharded run has waited for its collectives anyway)
    uint32_t bad = 0;
    HIPCHECK(d2h_small(cs, &bad, cs->d_small.p + kSensBadRecord, 4, s));
    auto check_records = [&]() -> int {
        if (bad & 1u) return fail(ctx, RALA_HIP_EINVAL, "sensitive overlap names must resolve");
        if (bad & 2u) return fail(ctx, RALA_HIP_EINVAL, "sensitive overlap targets a read that did not survive");
        return (int)RALA_HIP_OK;
    };
    if (sharded) {
        HIPCHECK(stream_sync(cs, s));
        HIPCHECK(hipGetLastError());
        const int rcb = check_records();
        if (rcb != RALA_HIP_OK) return rcb;
    }
    // bucketed by read on the pile holder: count -> scan -> scatter
    // (buffers of their own: the primary bound events stay where initialize left them)
    HIPCHECK(cl->d_sens_ev.ensure(n_tuples + 8));
    HIPCHECK(cl->d_sens_off.ensure(nl + 2));
    HIPCHECK(cl->d_sens_cur.ensure(nl + 2));
    HIPCHECK(cl->d_scan_ws.ensure(scan_workspace_bytes(std::max<uint64_t>(n_tuples, nl) + 2)));
    HIPCHECK(cl->d_dataset_median.ensure(nl));
    HIPCHECK(cl->d_n_rep.ensure(nl));
    HIPCHECK(cl->d_rep_slot.ensure(nl));
    cl->rep_pool_cap = std::max(cl->rep_pool_cap, cl->pool_cap_first);
    HIPCHECK(cl->d_rep_pool.ensure(cl->rep_pool_cap));
    if (sharded) {
        HIPCHECK(hipMemsetAsync(cl->d_n_rep.p, 0, nl * 4, sl));
        HIPCHECK(hipMemsetAsync(cl->d_small.p + kSensPoolCount, 0, kSensPoolWords * 4, sl));
    }
    if (sens_records) {
        // (the first pass' bucketing buffers have served: the bound events themselves stay where initialize left them)
        const uint32_t n_reads_l = (uint32_t)nl;
        HIPCHECK(cl->d_bk_u32[0].ensure(n_reads_l + 2));
        HIPCHECK(cl->d_bk_part.ensure(partition_count(n_reads_l, bt) + 2));
        HIPCHECK(cl->d_bk_group.ensure(3 * (size_t)partition_group_slots(n_reads_l, bt)));
        HIPCHECK(cl->d_bk_tiles.ensure(3 * partition_tile_slots(n_reads_l, n_sens, bt) + 2));
        for (int k = 0; k < 2; ++k) HIPCHECK(cl->d_bk_rec[k].ensure(partition_records_needed(n_reads_l, n_sens)));
        FillList fills;
        HIPCHECK(launch_bucket_partitioned_records(cs->d_sens_rec.p, n_sens, n_reads_l, bt, cl->d_bk_u32[0].p, cl->d_bk_part.p, cl->d_bk_group.p,
                                                   cl->d_bk_tiles.p, cl->d_bk_rec[0].p, cl->d_bk_rec[1].p, cl->d_sens_off.p, cl->d_sens_ev.p,
                                                   cl->n_compute_units, fills, sl, 0u, 0u));       // (the sensitive CSR: in events)
    } else {
        HIPCHECK(hipMemsetAsync(cl->d_sens_cur.p, 0, (nl + 1) * 4, sl));
        launch_count_tuples(tuples, n_tuples, (uint32_t)nl, cl->d_sens_cur.p, sl);
        launch_exclusive_scan(cl->d_sens_cur.p, cl->d_sens_off.p, nl, cl->d_scan_ws.p, sl);
        HIPCHECK(hipMemcpyAsync(cl->d_sens_cur.p, cl->d_sens_off.p, nl * 4, hipMemcpyDeviceToDevice, sl));
        launch_scatter_tuples(tuples, n_tuples, (uint32_t)nl, cl->d_sens_cur.p, cl->d_sens_ev.p, sl);
    }
    // the targets: reads that received bounds - listed where the offsets are, the host learns how many
    HIPCHECK(cl->d_sens_list.ensure(nl + 1));
    HIPCHECK(cl->d_chain_cnt.ensure(kChainWords));
    HIPCHECK(hipMemsetAsync(cl->d_chain_cnt.p + kChainTargets, 0, 4, sl));
    launch_list_targets(cl->d_sens_off.p, (uint32_t)nl, cl->d_sens_list.p, cl->d_chain_cnt.p + kChainTargets, sl);
    uint32_t n_targets = 0;
    uint32_t small[kSmallWords] = {};
    // (rows on demand: for the rest of this pass a target's row has these bounds on top; for the getters once the pass has
    // succeeded - the CSR then stays until the next rala_hip_initialize)
    struct PassRunning {
        rala_hip_ctx* c;
        explicit PassRunning(rala_hip_ctx* ctx_) : c(ctx_) { c->sens_pass_running = true; }
        ~PassRunning() { c->sens_pass_running = false; }
    } pass_running(cl);

    RepeatArgs a = repeat_args(cl);
    a.ev_off = cl->d_sens_off.p; a.ev = cl->d_sens_ev.p;
    // the same in run space: the primary events + the sensitive bounds
    PileArgs pa = pile_args(cl, primary_events(cl, cl->ev_fixed, cl->ev_shift));
    pa.stop_after = 99;
    pa.error = a.error;
    pa.sens_off = cl->d_sens_off.p; pa.sens_ev = cl->d_sens_ev.p;
    pa.dataset_median = a.dataset_median; pa.n_rep = a.n_rep; pa.rep_slot = a.rep_slot;
    pa.rep_pool = a.pool; pa.rep_pool_count = a.pool_count; pa.rep_pool_cap = a.pool_cap;
    // add_layers on top of the coverage + find_median for the targets (graph.cpp:941-969)
    int rc = run_sens_pass(cl, pa, a, 1, cl->d_sens_list.p, (uint32_t)nl, cl->d_chain_cnt.p + kChainTargets, &n_targets, small);
    if (!sharded) {
        // (the record check came back with the pass' first look; when the pass itself failed, a record that is an error is the
        // failure to report - the pass ran over what such records left behind: advisor round 5)
        const bool looked = rc == RALA_HIP_OK || stream_sync(cs, s) == hipSuccess;
        const int rcb = looked ? check_records() : (int)RALA_HIP_OK;
        if (rcb != RALA_HIP_OK) return rcb;
    }
    if (rc != RALA_HIP_OK) { if (cl != cs) cs->err = cl->err; return rc; }
    if (sharded) {
        // the new medians, everywhere
        HIPCHECK(cs->d_gather[0].ensure(nl_pad * 4 + 16));
        HIPCHECK(cs->d_gather[1].ensure(nl_pad * 4 * P + 16));
        launch_pack_median(cl->d_median.p, cl->d_p10.p, nl, nl_pad, (uint32_t*)cs->d_gather[0].p, s);
        if (comm->all_gather(cs->d_gather[0].p, cs->d_gather[1].p, nl_pad * 4, s) != 0) return comm_fail("all-gather of the medians");
        launch_unpack_median((const uint32_t*)cs->d_gather[1].p, P, nl_pad, n, cs->d_median.p, cs->d_p10.p, s);
    }
    if (!device_lists) {
        HIPCHECK(hipMemcpyAsync(cs->h_median.data(), cs->d_median.p, n * 2, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(cs->h_p10.data(), cs->d_p10.p, n * 2, hipMemcpyDeviceToHost, s));
        HIPCHECK(stream_sync(cs, s));
    }
    trc("rep: add_layers + median", n_targets);
    // first trim of the sensitive overlaps (graph.cpp:935-939)
    SensCoords sc;
    for (int k = 0; k < 5; ++k) HIPCHECK(cs->d_sens_c[k].ensure(n_sens));
    HIPCHECK(cs->d_sens_state.ensure(n_sens));
    sc.a_begin = cs->d_sens_c[0].p; sc.a_end = cs->d_sens_c[1].p; sc.b_begin = cs->d_sens_c[2].p;
    sc.b_end = cs->d_sens_c[3].p; sc.length = cs->d_sens_c[4].p; sc.state = cs->d_sens_state.p;
    launch_sens_trim(so, cs->d_sens_tb[0].p, cs->d_sens_tb[1].p, cs->d_begin.p, cs->d_end.p, cs->d_alive.p, sc, s);
    trc("rep: first trim", n_sens);
    // component medians over the primary overlaps -> repeat hills (graph.cpp:971-1026)
    std::vector<uint32_t> members;
    bool members_on_device = false;
    uint32_t n_members = 0;
    if (!device_lists) {
        std::vector<uint16_t> med;
        rc = component_medians(cs, members, med);
        if (rc != RALA_HIP_OK) return rc;
        std::vector<uint16_t> dm(n, 0);
        for (size_t k = 0; k < members.size(); ++k) dm[members[k]] = med[k];
        HIPCHECK(hipMemcpy(cs->d_dataset_median.p, dm.data(), n * 2, hipMemcpyHostToDevice));
    } else {
        // on the device list, in the rank space of the chimera stage (the new medians are in d_median)
        const TailList L = tail_list(cs);
        const uint32_t n_alive = cs->t_n_alive;
        rc = tail_components(cs, L, n_alive);
        if (rc != RALA_HIP_OK) return rc;
        HIPCHECK(hipMemsetAsync(cs->d_dataset_median.p, 0, n * 2, s));
        launch_scatter_component_medians(cs->d_alive_reads.p, cs->d_touched.p, cs->d_cmed.p, n_alive, cs->d_dataset_median.p, s);
        // the members (reads with an overlap; of a sharded run this rank's, as the owner's local ids) are listed where the
        // data is; the host learns how many
        HIPCHECK(cl->d_sens_list.ensure(std::max<uint64_t>(nl, 1) + 1));
        HIPCHECK(cs->d_chain_cnt.ensure(kChainWords));
        HIPCHECK(hipMemsetAsync(cs->d_chain_cnt.p + kChainMembers, 0, 4, s));
        launch_list_members(cs->d_alive_reads.p, cs->d_touched.p, n_alive, P, me, cl->d_sens_list.p, cs->d_chain_cnt.p + kChainMembers, s);
        if (sharded) HIPCHECK(stream_sync(cs, s));              // (the owner context's stream goes on from here)
        members_on_device = true;
    }
    std::vector<uint32_t> mine;
    if (sharded) {
        launch_localize_u16(cs->d_dataset_median.p, nl, P, me, cl->d_dataset_median.p, sl);
        if (!members_on_device) for (uint32_t r : members) if (r % P == me) mine.push_back(r / P);
    }
    uint32_t member_bound = (uint32_t)nl;
    if (!members_on_device) {
        // (host tail: the members were listed on the host)
        const std::vector<uint32_t>& list = sharded ? mine : members;
        HIPCHECK(cl->d_sens_list.ensure(std::max<uint64_t>(list.size(), 1) + 1));
        HIPCHECK(cs->d_chain_cnt.ensure(kChainWords));
        const uint32_t n_list = (uint32_t)list.size();
        if (n_list) HIPCHECK(hipMemcpy(cl->d_sens_list.p, list.data(), (size_t)n_list * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(cs->d_chain_cnt.p + kChainMembers, &n_list, 4, hipMemcpyHostToDevice));
        member_bound = n_list;
    }
    for (;;) {
        rc = run_sens_pass(cl, pa, a, 2, cl->d_sens_list.p, member_bound, cs->d_chain_cnt.p + kChainMembers, &n_members, small);
        if (rc != RALA_HIP_OK) { if (cl != cs) cs->err = cl->err; return rc; }
        if (!(small[kSensStatus] & kErrPoolCapacity)) break;
        // more repeat hills than the pool holds: its counter holds what is needed - the pass once more (mode 2 neither
        // reads nor writes the rows) with a pool of that size
        const uint32_t need = grown_pool_size(small[kSensPoolCount], cl->rep_pool_cap);
        if (!need) return fail(ctx, RALA_HIP_ENOMEM, "repeat-hill pool beyond 2^32 entries");
        cl->rep_pool_cap = need;
        HIPCHECK(cl->d_rep_pool.ensure(cl->rep_pool_cap));
        a.pool = cl->d_rep_pool.p; a.pool_cap = cl->rep_pool_cap;
        pa.rep_pool = cl->d_rep_pool.p; pa.rep_pool_cap = cl->rep_pool_cap;
        HIPCHECK(hipMemsetAsync(cl->d_n_rep.p, 0, nl * 4, sl));
        HIPCHECK(hipMemsetAsync(cl->d_small.p + kSensPoolCount, 0, kSensPoolWords * 4, sl));
        ++cl->tm.pool_regrown;
    }
    trc("rep: component medians + repeat hills", n_members);
    uint32_t n_hills = small[kSensPoolCount];
    if (sharded) {
        // capacity errors are everybody's; then the hills of all owners, slots rebased onto the
        // concatenation of their pools
        HIPCHECK(hipMemcpyAsync(cs->d_small.p + kSensStatus, &small[kSensStatus], 4, hipMemcpyHostToDevice, s));
        if (comm->all_reduce_u32(cs->d_small.p + kSensStatus, 1, ReduceOp::kMax, s) != 0) return comm_fail("all-reduce of the kernel status");
        HIPCHECK(d2h_small(cs, &small[kSensStatus], cs->d_small.p + kSensStatus, 4, s));
        HIPCHECK(stream_sync(cs, s));
    }
    if (small[kSensStatus] & (kErrRegionCapacity | kErrRawCapacity)) return fail(ctx, RALA_HIP_EDEVICE, "slope-region list overflow (repeat hills)");
    if (small[kSensStatus] & kErrPoolCapacity) return fail(ctx, RALA_HIP_EDEVICE, "repeat-hill pool exhausted");
    if (sharded) {
        const uint64_t mine = std::min<uint32_t>(small[kSensPoolCount], cl->rep_pool_cap);
        std::vector<uint64_t> counts(P);
        if (comm->host_all_gather(&mine, 1, counts.data(), s) != 0) return comm_fail("repeat-hill counts");
        RankOffsets base;
        uint64_t total = 0;
        for (uint32_t p = 0; p < P; ++p) { base.v[p] = (uint32_t)total; total += counts[p]; }
        HIPCHECK(cs->d_rep_pool.ensure(total + 1));
        HIPCHECK(cs->d_gather[0].ensure(nl_pad * 8 + 16));
        HIPCHECK(cs->d_gather[1].ensure(nl_pad * 8 * P + 16));
        launch_pack_rep(cl->d_n_rep.p, cl->d_rep_slot.p, nl, nl_pad, (uint64_t*)cs->d_gather[0].p, s);
        if (comm->all_gather(cs->d_gather[0].p, cs->d_gather[1].p, nl_pad * 8, s) != 0) return comm_fail("all-gather of the repeat hills");
        launch_unpack_rep((const uint64_t*)cs->d_gather[1].p, P, nl_pad, n, base, cs->d_n_rep.p, cs->d_rep_slot.p, s);
        if (comm->all_gather_v(cl->d_rep_pool.p, cs->d_rep_pool.p, counts.data(), sizeof(Interval), s) != 0) {
            return comm_fail("all-gather of the repeat-hill pools");
        }
        n_hills = (uint32_t)total;
    }
    trc("rep: repeat hills kernel", n_hills);
    // sensitive dovetails mark the hills they bridge (graph.cpp:1028-1043)
    launch_sens_bridge(so, sc, cs->d_begin.p, cs->d_end.p, cs->d_alive.p, cs->d_n_rep.p, cs->d_rep_slot.p,
                       cs->d_rep_pool.p, s);
    if (sharded && n_hills) {
        HIPCHECK(cs->d_t_tmp[0].ensure(std::max<size_t>(n_hills, n) + 2));
        launch_pool_aux(cs->d_rep_pool.p, n_hills, cs->d_t_tmp[0].p, 0, s);
        if (comm->all_reduce_u32(cs->d_t_tmp[0].p, n_hills, ReduceOp::kMax, s) != 0) return comm_fail("all-reduce of the bridged flags");
        launch_pool_aux(cs->d_rep_pool.p, n_hills, cs->d_t_tmp[0].p, 1, s);
    }
    if (sharded || trc.on) {                    // (one context: the next look is the graph's, gpu_tail_part_b)
        HIPCHECK(stream_sync(cs, s));
        HIPCHECK(hipGetLastError());
    }
    trc("rep: bridged hills", n_sens);
    // the host's copy of the hills: at once where the host filters the overlaps below, otherwise with the first getter
    repeat_hills_left_on_device(cs, n_hills);
    if (!device_lists) {
        const int rcd = download_repeat_hills(cs);
        if (rcd != RALA_HIP_OK) return rcd;
    }
    trc("rep: download hills", n_hills);
    // overlaps that end inside a bridged edge hill are dropped (graph.cpp:1045-1051)
    if (device_lists) {
        launch_sens_filter(tail_list(cs), cs->d_begin.p, cs->d_end.p, cs->d_n_rep.p, cs->d_rep_slot.p, cs->d_rep_pool.p, s);
    } else {
        size_t w = 0;
        for (size_t k = 0; k < cs->overlaps.size(); ++k) {
            const HostOvl& o = cs->overlaps[k];
            if (!is_valid_overlap(cs, o.a, o.c.a_begin, o.c.a_end) ||
                !is_valid_overlap(cs, o.b, o.c.b_begin, o.c.b_end)) {
                continue;
            }
            if (w != k) cs->overlaps[w] = cs->overlaps[k];
            ++w;
        }
        cs->overlaps.resize(w);
    }
    trc("rep: filter overlaps", cs->overlaps.size());
    repeat_hills_found(cs);
    sensitive_bounds_kept(cl);
    return RALA_HIP_OK;
}

int rala_hip::repeats_stage(rala_hip_ctx* cs, rala_hip_ctx* cl, Comm* comm, const rala_hip_overlaps* sens, uint64_t n_sens) {
    if (!cs || !cl) return RALA_HIP_EINVAL;
    if (!cs->constructed) return fail(cs, RALA_HIP_EINVAL, "construct_stages must have run");
    if (!cl->piles_resident) return fail(cs, RALA_HIP_EINVAL, "the sensitive pass needs the piles on the owner context");
    const double t0 = now_ms();
    const int rc = repeats_after_tail(cs, cl, comm, sens, n_sens);
    cs->tm.repeats_ms = (float)(now_ms() - t0);
    cs->tm.tail_host_ms += cs->tm.repeats_ms;
    return rc;
}

extern "C" {

int rala_hip_find_repetitive_hills(rala_hip_ctx* ctx, uint64_t read, uint32_t begin, uint32_t end, uint16_t median,
                                   uint16_t p10, uint16_t dataset_median) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!ctx->initialized || read >= ctx->n_reads) return fail(ctx, RALA_HIP_EINVAL, "bad read / not initialized");
    if (!ctx->piles_resident) return fail(ctx, RALA_HIP_EINVAL, "the piles live on another context");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    if (!ctx->h_alive[read]) return fail(ctx, RALA_HIP_EINVAL, "the read was filtered");
    if (begin > end || end > ctx->h_read_len[read]) return fail(ctx, RALA_HIP_EINVAL, "bad valid region");
    ctx->h_begin[read] = begin; ctx->h_end[read] = end; ctx->h_median[read] = median; ctx->h_p10[read] = p10;
    const uint64_t n = ctx->n_reads;
    hipStream_t s = ctx->stream;
    HIPCHECK(ctx->d_dataset_median.ensure(n));
    HIPCHECK(ctx->d_n_rep.ensure(n));
    HIPCHECK(ctx->d_rep_slot.ensure(n));
    ctx->rep_pool_cap = std::max(ctx->rep_pool_cap, ctx->pool_cap_first);
    HIPCHECK(ctx->d_rep_pool.ensure(ctx->rep_pool_cap));
    if (!ctx->have_repeats) {
        HIPCHECK(hipMemsetAsync(ctx->d_n_rep.p, 0, n * 4, s));
        HIPCHECK(hipMemsetAsync(ctx->d_small.p + kSensPoolCount, 0, kSensPoolWords * 4, s));
        ctx->h_n_rep.assign(n, 0); ctx->h_rep_slot.assign(n, 0); ctx->h_rep_pool.clear();
    }
    // the valid region as it stands (the host mirrors are authoritative after a host tail)
    HIPCHECK(hipMemcpyAsync(ctx->d_begin.p + read, &ctx->h_begin[read], 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_end.p + read, &ctx->h_end[read], 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_median.p + read, &ctx->h_median[read], 2, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_p10.p + read, &ctx->h_p10[read], 2, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_dataset_median.p + read, &dataset_median, 2, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(ctx->d_small.p + kSensStatus, 0, 4, s));
    HIPCHECK(stream_sync(ctx, s));
    RepeatArgs a = repeat_args(ctx);
    a.ev_off = ctx->d_ev_off.p; a.ev = ctx->d_ev.p;
    const std::vector<uint32_t> one(1, (uint32_t)read);
    uint32_t small[kSensStatus + 1];            // d_small up to the status
    for (;;) {
        uint32_t used_before = 0;
        HIPCHECK(hipMemcpy(&used_before, ctx->d_small.p + kSensPoolCount, 4, hipMemcpyDeviceToHost));
        const int rc = run_repeats_kernel(ctx, a, one, 2);
        if (rc != RALA_HIP_OK) return rc;
        HIPCHECK(hipMemcpy(small, ctx->d_small.p, sizeof(small), hipMemcpyDeviceToHost));
        if (!(small[kSensStatus] & kErrPoolCapacity)) break;
        // the pool (it keeps the hills of earlier calls) is too small for this read's: a larger one, the call once more
        const uint32_t need = grown_pool_size(small[kSensPoolCount], ctx->rep_pool_cap);
        if (!need) return fail(ctx, RALA_HIP_ENOMEM, "repeat-hill pool beyond 2^32 entries");
        rala_hip::DevBuf<Interval> larger;
        HIPCHECK(larger.ensure(need));
        if (used_before) HIPCHECK(hipMemcpy(larger.p, ctx->d_rep_pool.p, (size_t)used_before * sizeof(Interval), hipMemcpyDeviceToDevice));
        std::swap(larger.p, ctx->d_rep_pool.p);
        std::swap(larger.n, ctx->d_rep_pool.n);
        ctx->rep_pool_cap = need;
        a.pool = ctx->d_rep_pool.p; a.pool_cap = ctx->rep_pool_cap;
        const uint32_t reset[kSensPoolWords] = {used_before, 0};                // (the pool's count as it was, no status)
        HIPCHECK(hipMemcpy(ctx->d_small.p + kSensPoolCount, reset, sizeof(reset), hipMemcpyHostToDevice));
    }
    if (small[kSensStatus] & (kErrRegionCapacity | kErrRawCapacity)) return fail(ctx, RALA_HIP_EDEVICE, "slope-region list overflow (repeat hills)");
    ctx->h_n_rep.resize(n); ctx->h_rep_slot.resize(n);
    HIPCHECK(hipMemcpy(&ctx->h_n_rep[read], ctx->d_n_rep.p + read, 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(&ctx->h_rep_slot[read], ctx->d_rep_slot.p + read, 4, hipMemcpyDeviceToHost));
    ctx->h_rep_pool.resize(small[kSensPoolCount]);
    if (small[kSensPoolCount]) HIPCHECK(hipMemcpy(ctx->h_rep_pool.data(), ctx->d_rep_pool.p, (size_t)small[kSensPoolCount] * sizeof(Interval), hipMemcpyDeviceToHost));
    ctx->n_rep_hills = small[kSensPoolCount];
    repeat_hills_fetched(ctx);
    repeat_hills_found(ctx);
    return RALA_HIP_OK;
}

}  // extern "C"
