// librala_hip: Graph::preprocess for chimeras and the graph behind it with the survivor lists resident on the device
// (tail_kernels.hip), and the host's mirrors of that result.  Implements no call of rala_hip.h by itself: construct.hip,
// sensitive.hip, transitive.hip and getters.hip call it (orchestration.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "lifecycle.h"
#include "orchestration.h"
#include "scan_pass.h"

using namespace rala_hip;

// ---- preprocess tail on the device (tail_kernels.hip) ---------------------------------------
// the ten columns of the survivor lists (d_surv_u32[0..7], d_surv_u8[0..1], or host copies of them) in the order of
// Survivors' members
Survivors rala_hip::survivors_of(uint32_t* const c32[8], uint8_t* strand, uint8_t* type) {
    return Survivors{c32[0], c32[1], c32[2], c32[3], c32[4], c32[5], c32[6], c32[7], strand, type};
}
Survivors rala_hip::survivors_view(rala_hip_ctx* ctx) {
    uint32_t* c32[8];
    for (int f = 0; f < 8; ++f) c32[f] = ctx->d_surv_u32[f].p;
    return survivors_of(c32, ctx->d_surv_u8[0].p, ctx->d_surv_u8[1].p);
}

// item k of survivor columns on the host, as the host lists hold it
HostOvl rala_hip::host_item(const Survivors& sv, size_t k) {
    HostOvl o;
    o.src = sv.src[k]; o.a = sv.a_id[k]; o.b = sv.b_id[k];
    o.c.a_begin = sv.a_begin[k]; o.c.a_end = sv.a_end[k]; o.c.b_begin = sv.b_begin[k]; o.c.b_end = sv.b_end[k]; o.c.length = sv.length[k];
    o.strand = sv.strand[k]; o.dead = 0; o.type = sv.type[k];
    return o;
}

TailList rala_hip::tail_list(rala_hip_ctx* ctx) {
    const Survivors sv = survivors_view(ctx);
    TailList L;
    L.n = ctx->t_n0 + ctx->t_n1;
    L.src = sv.src; L.a = sv.a_id; L.b = sv.b_id; L.a_begin = sv.a_begin; L.a_end = sv.a_end; L.b_begin = sv.b_begin;
    L.b_end = sv.b_end; L.length = sv.length; L.strand = sv.strand; L.type = sv.type;
    L.state = ctx->d_t_state.p; L.round = ctx->d_t_round.p;
    return L;
}

namespace {

TailReads tail_reads(rala_hip_ctx* ctx) {
    TailReads R;
    R.begin = ctx->d_begin.p; R.end = ctx->d_end.p; R.alive = ctx->d_alive.p; R.dirty = ctx->d_dirty.p;
    R.n_pits = ctx->d_n_pits.p; R.n_hills = ctx->d_n_hills.p; R.n_pits0 = ctx->d_n_pits0.p;
    R.iv_slot = ctx->d_iv_slot.p; R.pool = ctx->d_pool.p;
    return R;
}

}  // namespace

// tile states for the single-pass scans of one stage (scan_pass.h): `scans` scans of up to `items` items;
// cleared (with the ticket counter behind them) by one fill - the caller's list of fills if it has one
int rala_hip::scan_space(rala_hip_ctx* ctx, uint32_t scans, uint64_t items, ScanSpace& sp, FillList* fills) {
    const size_t words = (size_t)scans * (scan_tiles_for(items) + 2) + 2;
    HIPCHECK(ctx->d_scan_state.ensure(words));
    sp.state = ctx->d_scan_state.p;
    sp.words = words - 2;
    sp.used = 0;
    sp.ticket = (uint32_t*)(ctx->d_scan_state.p + words - 2);
    if (fills) fills->add(ctx->d_scan_state.p, 0, words * 8);
    else HIPCHECK(hipMemsetAsync(ctx->d_scan_state.p, 0, words * 8, ctx->stream));
    return RALA_HIP_OK;
}

// connected components over the live overlaps of the device list (labels in the rank space of
// d_rank / d_alive_reads) and, per read with an overlap, the median of the pile medians of its
// component (graph.cpp:740-783): d_touched[rank], d_cmed[rank]
// (touched_cleared: the caller's fill has zeroed d_touched)
int rala_hip::tail_components(rala_hip_ctx* ctx, const TailList& L, uint32_t n_alive, bool touched_cleared) {
    hipStream_t s = ctx->stream;
    const uint32_t M = L.n;
    if (!touched_cleared) {
        FillList fills;
        fills.add(ctx->d_touched.p, 0, n_alive);
        component_median_clear(ctx->d_med_tmp.p, n_alive, fills);
        HIPCHECK(fills.launch(s));
    }
    launch_cc_edges(L, ctx->d_rank.p, ctx->d_cc_edges.p, ctx->d_touched.p, ctx->d_cc_label.p, n_alive, s);
    for (int k = 0; k < 2; ++k) {                               // sampled rounds, see cc_hook_kernel
        launch_cc_hook(ctx->d_cc_edges.p, M, 1, ctx->d_cc_label.p, ctx->d_cc_flags.p + kCcTailChanged, s);
        launch_cc_compress(ctx->d_cc_label.p, n_alive, s);
    }
    // one launch over all edges finishes the components (cc_hook_kernel unites to the end); the last compression
    // counts the components' reads with an overlap
    launch_cc_hook(ctx->d_cc_edges.p, M, 0, ctx->d_cc_label.p, ctx->d_cc_flags.p + kCcTailChanged, s);
    launch_cc_compress_count(ctx->d_cc_label.p, n_alive, ctx->d_touched.p, component_median_sizes(ctx->d_med_tmp.p, n_alive), s);
    // median of the pile medians per component (graph.cpp:777-783)
    HIPCHECK(launch_component_medians(ctx->d_cc_label.p, ctx->d_touched.p, ctx->d_alive_reads.p, ctx->d_median.p, n_alive,
                                      ctx->d_med_tmp.p, ctx->d_cmed.p, s));
    return RALA_HIP_OK;
}

// Graph::preprocess (chimeras) with the survivor lists resident on the device: everything up to
// and including the in-order containment removal (graph.cpp:699-877)
int rala_hip::gpu_tail_part_a(rala_hip_ctx* ctx) {
    hipStream_t s = ctx->stream;
    Trace trc;
    auto mark = [&](const char* what, size_t k = 0) {
        if (trc.on) { (void)stream_sync(ctx, s); trc(what, k); }
    };
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    const uint32_t M = ctx->t_n0 + ctx->t_n1;
    // (how many reads are alive came back with the survivor counts of the second pass: no look from the host here)
    const uint32_t n_alive = ctx->t_n_alive;
    HIPCHECK(ctx->d_t_state.ensure(M)); HIPCHECK(ctx->d_t_round.ensure(M));
    HIPCHECK(ctx->d_dirty.ensure(n_reads)); HIPCHECK(ctx->d_n_pits0.ensure(n_reads));
    HIPCHECK(ctx->d_rank.ensure(n_reads)); HIPCHECK(ctx->d_alive_reads.ensure(n_reads));
    HIPCHECK(ctx->d_kept_item.ensure(M));
    HIPCHECK(ctx->d_node_rank.ensure(n_reads + 2)); HIPCHECK(ctx->d_t_death[0].ensure(n_reads));
    HIPCHECK(ctx->d_t_death[1].ensure(n_reads));
    HIPCHECK(ctx->d_touched.ensure(n_alive)); HIPCHECK(ctx->d_cmed.ensure(n_alive));
    HIPCHECK(ctx->d_cc_edges.ensure(2 * (size_t)M)); HIPCHECK(ctx->d_cc_label.ensure(n_alive));
    ctx->t_med_tmp = component_median_workspace(n_alive);
    HIPCHECK(ctx->d_med_tmp.ensure(ctx->t_med_tmp));
    HIPCHECK(ctx->d_cc_flags.ensure(kCcFlagsWords));
    // (the containment scans order the items by key = items * (1 + round of promotion) + index, 32 bits: checked below with the
    // rounds this data set took - two to four - and not with the 255 a round counter could hold; before round 5 that was a
    // limit of 16.6 M surviving overlaps, 2.2 times C5's)
    if ((uint64_t)M >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "too many surviving overlaps");
    const TailList L = tail_list(ctx);
    const TailReads R = tail_reads(ctx);
    ScanSpace sp;
    {
        FillList fills;
        const int rc = scan_space(ctx, 1, n_reads, sp, &fills);
        if (rc != RALA_HIP_OK) return rc;
        HIPCHECK(fills.launch(s));
    }
    // (d_counts: cleared by the second pass; the tail's words are TailCounts, slots.h)
    HIPCHECK(ctx->d_counts.ensure(kCountsWords));
    for (int k = 0; k < 2; ++k) HIPCHECK(ctx->d_t_work[k].ensure(n_reads));
    HIPCHECK(ctx->d_t_fin.ensure(2 * (size_t)n_reads));
    HIPCHECK(ctx->d_t_mark.ensure(2 * (size_t)n_reads));
    for (int k = 0; k < 3; ++k) { HIPCHECK(ctx->d_kill[k].ensure((size_t)M + 1)); HIPCHECK(ctx->d_kill2[k].ensure((size_t)M + 1)); }
    HIPCHECK(ctx->d_fp_map.ensure(n_reads));
    HIPCHECK(ctx->d_fp_pack.ensure(fixed_point_pack_words()));
    launch_tail_init(L, ctx->t_n0, R, ctx->d_n_pits0.p, n_reads, ctx->d_t_fin.p, ctx->d_t_mark.p, ctx->d_fp_map.p, ctx->d_counts.p + kTailContain, s);
    // ranks of the reads that survived the second pass (the component graph lives on them)
    if (!launch_rank_pass(ctx->d_alive.p, ctx->d_rank.p, ctx->d_alive_reads.p, n_reads, sp, s)) return fail(ctx, RALA_HIP_EDEVICE, "scan space");
    mark("tail: ranks", n_alive);

    // break over chimeric hills, first re-trim (graph.cpp:704-736; no promotion here)
    uint32_t* dropped = ctx->d_counts.p + kTailDropped;             // one word per round of a batch
    launch_break_hills(R, n_reads, s);
    if (ctx->lists_pending) {           // (a sharded run's survivor lists, gathered beside the kernels above)
        HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvGatherJoin], 0));
        ctx->lists_pending = false;
    }
    launch_retrim(L, R, 0, 0, dropped, s);
    mark("tail: hills + retrim", M);

    // graph.cpp:738-829: components, component medians, break over pits, re-trim - while an overlap died
    // in the round.  Hardly a data set is done after one round, and a look from the host costs a third of
    // one: two rounds are enqueued before the host looks, the second one gated on the device by the first
    // one's count (a round behind the reference's last would see the internals that round promoted as
    // overlaps - it must not act), then one at a time.
    uint32_t rounds = 0;
    for (;;) {
        const uint32_t batch = rounds == 0 ? 2u : 1u;
        for (uint32_t k = 0; k < batch; ++k) {
            if (rounds + k >= 255) return fail(ctx, RALA_HIP_EDEVICE, "chimera loop did not settle");
            const uint32_t* gate = k ? dropped + k - 1 : nullptr;
            // one fill: the dirt the last re-trim has dealt with, the components' marks, the batch's verdicts
            FillList fills;
            fills.add(ctx->d_dirty.p, 0, n_reads);
            fills.add(ctx->d_touched.p, 0, n_alive);
            component_median_clear(ctx->d_med_tmp.p, n_alive, fills);
            if (k == 0) fills.add(dropped, 0, kTailDroppedWords * 4);
            HIPCHECK(fills.launch(s));
            const int rcc = tail_components(ctx, L, n_alive, true);
            if (rcc != RALA_HIP_OK) return rcc;
            launch_break_pits(R, ctx->d_alive_reads.p, ctx->d_touched.p, ctx->d_cmed.p, n_alive, s, gate);
            launch_retrim(L, R, 1, rounds + k, dropped + k, s, gate);
        }
        uint32_t d[kTailDroppedWords] = {};
        HIPCHECK(d2h_small(ctx, d, dropped, sizeof(d), s));
        HIPCHECK(stream_sync(ctx, s));
        mark("tail: pits + retrim", d[0] + d[1]);
        if (!d[0]) { rounds += 1; break; }                     // (a second round of the batch did nothing)
        rounds += batch;
        if (!d[batch - 1]) break;
    }
    ctx->t_rounds = rounds;
    if ((uint64_t)M * ((uint64_t)rounds + 2ull) >= 0xFFFFFFF0ull) {
        return fail(ctx, RALA_HIP_ETOOLARGE, "too many surviving overlaps for 32-bit list positions");
    }

    // in-order containment removal (graph.cpp:831-877): overlaps (+ promoted), then internals
    {
        uint32_t* const work[4] = {ctx->d_t_death[0].p, ctx->d_t_death[1].p, ctx->d_t_work[0].p, ctx->d_t_work[1].p};
        uint32_t* const lists[6] = {ctx->d_kill[0].p, ctx->d_kill[1].p, ctx->d_kill[2].p, ctx->d_kill2[0].p, ctx->d_kill2[1].p,
                                    ctx->d_kill2[2].p};
        HIPCHECK(launch_tail_contain(L, R, ctx->d_alive.p, lists, ctx->d_counts.p + kTailContain, work, ctx->d_t_fin.p, ctx->d_t_mark.p, ctx->d_fp_map.p,
                                     ctx->d_fp_pack.p, n_reads, ctx->debug_fp_lds_limit, ctx->debug_fp_give_up, s));
    }
    mark("tail: containment scans", M);
    return RALA_HIP_OK;
}

// ... the final overlap list, nodes and edges (graph.cpp:553-632, :869-877) from the device list
int rala_hip::gpu_tail_part_b(rala_hip_ctx* ctx) {
    hipStream_t s = ctx->stream;
    Trace trc;
    auto mark = [&](const char* what, size_t k = 0) {
        if (trc.on) { (void)stream_sync(ctx, s); trc(what, k); }
    };
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    const uint32_t M = ctx->t_n0 + ctx->t_n1;
    const TailList L = tail_list(ctx);
    const TailReads R = tail_reads(ctx);
    const uint32_t n_seg = ctx->t_rounds + 1;
    // sized by what the host knows: at most t_n_alive reads are left, at most M overlaps kept, all dovetails
    HIPCHECK(ctx->d_seg_base.ensure(2 * (size_t)n_seg + 4));
    HIPCHECK(ctx->d_node_read.ensure(2 * (size_t)ctx->t_n_alive + 2));
    for (int k = 0; k < 3; ++k) HIPCHECK(ctx->d_e[k].ensure(2 * (size_t)M + 2));
    ScanSpace sp;
    {
        FillList fills;
        const int rc = scan_space(ctx, n_seg + 1, std::max<uint64_t>(n_reads, M), sp, &fills);
        if (rc != RALA_HIP_OK) return rc;
        fills.add(ctx->d_seg_base.p, 0, (2 * (size_t)n_seg + 4) * 4);
        fills.add(ctx->d_counts.p + kTailReadsLeft, 0, 4);
        HIPCHECK(fills.launch(s));
    }
    // nodes: two per surviving read (graph.cpp:553-574)
    if (!launch_node_pass(ctx->d_alive.p, ctx->d_node_rank.p, ctx->d_node_read.p, ctx->d_counts.p + kTailReadsLeft, n_reads, sp, s)) {
        return fail(ctx, RALA_HIP_EDEVICE, "scan space");
    }
    // the final overlap list: originals in order, then the promoted ones round by round; the two edges of
    // every dovetail (graph.cpp:576-632) with it
    for (uint32_t seg = 0; seg < n_seg; ++seg) {
        // (the last segment's sums - the totals - go next to the other counts the host fetches: kTailTotals)
        if (!launch_segment_pass(L, R, seg == 0 ? 1u : 3u, seg == 0 ? 0u : seg - 1, ctx->d_seg_base.p + 2 * seg,
                                 seg + 1 == n_seg ? ctx->d_counts.p + kTailTotals : ctx->d_seg_base.p + 2 * (seg + 1), ctx->d_kept_item.p,
                                 ctx->d_node_rank.p, ctx->d_e[0].p,
                                 ctx->d_e[1].p, ctx->d_e[2].p, sp, s)) {
            return fail(ctx, RALA_HIP_EDEVICE, "scan space");
        }
    }
    struct { uint32_t kept, dovetails, reads_left, scan_failed; } look = {};       // kTailTotals .. kTailContain, one copy
    static_assert(sizeof(look) == kTailLookWords * 4, "one word per count");
    HIPCHECK(d2h_small(ctx, &look, ctx->d_counts.p + kTailTotals, sizeof(look), s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    if (trace_on()) {
        struct { uint32_t ov, in, ov_conditional, in_conditional; } killers = {};
        static_assert(sizeof(killers) == kTailKillerWords * 4, "one word per count");
        HIPCHECK(hipMemcpy(&killers, ctx->d_counts.p + kTailKillers, sizeof(killers), hipMemcpyDeviceToHost));
        fprintf(stderr, "[trace] tail containment killers: %u (%u conditional) among the overlaps, %u (%u) among the internals, of %u items\n",
                killers.ov, killers.ov_conditional, killers.in, killers.in_conditional, M);
    }
    if (look.scan_failed) {
        return fail(ctx, RALA_HIP_EDEVICE, "containment fixed point did not converge");
    }
    ctx->t_n_kept = look.kept;
    ctx->t_n_nodes = 2 * look.reads_left;
    ctx->t_n_edges = 2 * look.dovetails;
    mark("tail: final list, nodes, edges", ctx->t_n_edges);
    tail_left_on_device(ctx);
    return RALA_HIP_OK;
}

int rala_hip::gpu_tail_run(rala_hip_ctx* ctx) {
    const int rc = gpu_tail_part_a(ctx);
    return rc != RALA_HIP_OK ? rc : gpu_tail_part_b(ctx);
}

// host mirrors of a device-resident result (lists in the reference's order, graph, read state)
int rala_hip::materialize_host(rala_hip_ctx* ctx) {
    if (ctx->have_repeats && ctx->rep_host_stale) {
        const int rcr = download_repeat_hills(ctx);
        if (rcr != RALA_HIP_OK) return rcr;
    }
    if (!ctx->host_stale) return ctx->host_state_fresh ? RALA_HIP_OK : download_read_state(ctx);
    hipStream_t s = ctx->stream;
    int rc = download_read_state(ctx);
    if (rc != RALA_HIP_OK) return rc;
    const uint32_t M = ctx->t_n0 + ctx->t_n1;
    std::vector<uint32_t> h[8];
    std::vector<uint8_t> strand(M), type(M), state(M);
    uint32_t* c32[8];
    for (int f = 0; f < 8; ++f) {
        h[f].resize(M);
        c32[f] = h[f].data();
        if (M) HIPCHECK(hipMemcpyAsync(h[f].data(), ctx->d_surv_u32[f].p, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    }
    std::vector<uint32_t> kept(ctx->t_n_kept);
    if (M) {
        HIPCHECK(hipMemcpyAsync(strand.data(), ctx->d_surv_u8[0].p, M, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(type.data(), ctx->d_surv_u8[1].p, M, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(state.data(), ctx->d_t_state.p, M, hipMemcpyDeviceToHost, s));
    }
    if (ctx->t_n_kept) {
        HIPCHECK(hipMemcpyAsync(kept.data(), ctx->d_kept_item.p, (size_t)ctx->t_n_kept * 4, hipMemcpyDeviceToHost, s));
    }
    ctx->node_read.resize(ctx->t_n_nodes);
    ctx->e_src.resize(ctx->t_n_edges); ctx->e_dst.resize(ctx->t_n_edges); ctx->e_len.resize(ctx->t_n_edges);
    if (ctx->t_n_nodes) {
        HIPCHECK(hipMemcpyAsync(ctx->node_read.data(), ctx->d_node_read.p, (size_t)ctx->t_n_nodes * 4, hipMemcpyDeviceToHost, s));
    }
    if (ctx->t_n_edges) {
        HIPCHECK(hipMemcpyAsync(ctx->e_src.data(), ctx->d_e[0].p, (size_t)ctx->t_n_edges * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(ctx->e_dst.data(), ctx->d_e[1].p, (size_t)ctx->t_n_edges * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(ctx->e_len.data(), ctx->d_e[2].p, (size_t)ctx->t_n_edges * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(stream_sync(ctx, s));
    ctx->e_mark.assign(ctx->t_n_edges, 0);
    const Survivors sv = survivors_of(c32, strand.data(), type.data());
    ctx->overlaps.clear(); ctx->internals.clear();
    for (uint32_t k : kept) ctx->overlaps.push_back(host_item(sv, k));
    for (uint32_t k = ctx->t_n0; k < M; ++k) if (state[k] == 2) ctx->internals.push_back(host_item(sv, k));
    host_lists_fetched(ctx);
    return RALA_HIP_OK;
}
