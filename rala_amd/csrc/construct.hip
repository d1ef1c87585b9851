// librala_hip: the second overlap pass and what follows it.  Implements rala_hip_construct of rala_hip.h and construct_stages
// of stages.h; the chimera stage and the graph are tail_device.hip's (use_gpu_tail = 0: tail_host.hip's), the sensitive pass
// sensitive.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "lifecycle.h"
#include "orchestration.h"
#include "scan_pass.h"

using namespace rala_hip;

namespace {

ReadState read_state(rala_hip_ctx* ctx) {
    ReadState rs;
    rs.begin = ctx->d_begin.p; rs.end = ctx->d_end.p; rs.alive = ctx->d_alive.p;
    rs.n_pits = ctx->d_n_pits.p; rs.n_hills = ctx->d_n_hills.p; rs.iv_slot = ctx->d_iv_slot.p;
    rs.pool = ctx->d_pool.p;
    return rs;
}

// ---- sharded survivor lists: a rank's survivors travel as one packed block -------------------
// block of m items: eight uint32 columns (src, a, b, a_begin, a_end, b_begin, b_end, length) of m
// entries each, then the strand and type bytes; overlaps first, internals behind them
size_t packed_list_bytes(uint64_t m) { return ((size_t)m * 34 + 15) & ~(size_t)15; }

Survivors packed_list_view(uint8_t* block, uint64_t m) {
    Survivors sv;
    uint32_t* c = (uint32_t*)block;
    sv.src = c; sv.a_id = c + m; sv.b_id = c + 2 * m; sv.a_begin = c + 3 * m; sv.a_end = c + 4 * m;
    sv.b_begin = c + 5 * m; sv.b_end = c + 6 * m; sv.length = c + 7 * m;
    sv.strand = block + 32 * m; sv.type = block + 33 * m;
    return sv;
}

// Second overlap pass on ctx->ovl (graph.cpp:443-518): static classification, the in-order
// containment removal as a fixed point, liveness + hill counters, survivors into the tail lists
// (ctx->d_surv_*, t_n0 overlaps then t_n1 internals).  With a communicator the overlaps are one
// slice of the file: the bounds of the fixed point are all-reduced (min) per round, the hill
// counters all-reduced (sum), the survivor lists all-gathered in slice (= file) order.
int pass2(rala_hip_ctx* ctx, Comm* comm) {
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    const uint64_t N = ctx->n_ovl;
    const ReadState rs = read_state(ctx);
    auto comm_fail = [&](const char* what) {
        ctx->err = std::string(what) + ": " + comm->error();
        ctx->stage_pending.clear();
        ctx->stage_used = 0;
        return RALA_HIP_EDEVICE;
    };

    if (ctx->dedupe_pending) {          // (a sharded run's duplicate removal ran beside the emit, on the side stream)
        HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvEmitDedupeDone], 0));
        dedupe_joined(ctx);
    }
    // ---- static part ----
    // (a sharded run gathers up to 65 536 undecided killers of ALL ranks on every rank: room for them whatever the slice's size)
    const uint64_t kill_room = comm ? std::max<uint64_t>(N + 1, (1u << 16) + 1) : N + 1;
    for (int k = 0; k < 3; ++k) HIPCHECK(ctx->d_kill[k].ensure(kill_room));
    // the killer lists' counters: a fresh, pre-zeroed one per round of the fixed point
    constexpr uint32_t kCountRing = 128;
    HIPCHECK(ctx->d_kill_count.ensure(kCountRing + 4));
    KillList kl;
    kl.count = ctx->d_kill_count.p; kl.ovl = ctx->d_kill[0].p; kl.target = ctx->d_kill[1].p; kl.keeper = ctx->d_kill[2].p;
    HIPCHECK(hipEventRecord(ctx->ev[kEvPass2Begin], s));
    HIPCHECK(ctx->d_rec.ensure(n_reads));
    // compact per-read records (valid region + two flags): 4 bytes when no read is longer than 32767 bases
    const bool small_rec = ctx->max_read_len <= 32767u;
    HIPCHECK(ctx->d_crec.ensure((size_t)n_reads * compact_record_bytes(small_rec) + 16));
    HIPCHECK(ctx->d_counts.ensure(kCountsWords));
    // one buffer: sure[n_reads] (min over sure killers = upper bound), lo[n_reads] (lower bound),
    // one status word - so that a sharded run needs ONE all-reduce (min) per round; up[] apart
    HIPCHECK(ctx->d_death_sure.ensure(2 * (size_t)n_reads + 8));
    HIPCHECK(ctx->d_fp_map.ensure(n_reads));
    HIPCHECK(ctx->d_fp_pack.ensure(fixed_point_pack_words()));
    uint32_t* sure = ctx->d_death_sure.p;
    uint32_t* lo = sure + n_reads;
    const size_t dbytes = (size_t)n_reads * 4;
    ScanSpace chunk_scan;
    {
        FillList fills;
        const int rc = scan_space(ctx, 1, pass2_chunks(N), chunk_scan, &fills);
        if (rc != RALA_HIP_OK) return rc;
        fills.add(ctx->d_kill_count.p, 0, (kCountRing + 4) * 4);
        fills.add(ctx->d_counts.p, 0, kCountsWords * 4);
        fills.add(sure, 0xFF, 2 * dbytes + 4);
        fills.add(ctx->d_fp_map.p, 0xFF, dbytes);               // (launch_fixed_point_finish leaves it that way; here for good measure)
        HIPCHECK(fills.launch(s));
    }
    // (tests: a failure that only this rank sees, between two collectives of a sharded run)
    if (ctx->debug_fail_construct) return fail(ctx, RALA_HIP_EDEVICE, "debug_fail_construct");
    launch_pack_reads(rs, n_reads, ctx->d_rec.p, ctx->d_crec.p, small_rec, sure, s);
    launch_classify(ctx->ovl, n_reads, ctx->d_valid.p, ctx->d_crec.p, small_rec, kl, lo, s);
    HIPCHECK(hipEventRecord(ctx->ev[kEvPass2Classified], s));

    // ---- in-order containment removal as a fixed point (death_decide_kernel) ----
    for (int k = 0; k < 3; ++k) HIPCHECK(ctx->d_kill2[k].ensure(kill_room));
    KillList klist[2] = {kl, kl};
    uint32_t next_count = 1;
    klist[1].ovl = ctx->d_kill2[0].p; klist[1].target = ctx->d_kill2[1].p; klist[1].keeper = ctx->d_kill2[2].p;
    uint32_t* status = sure + 2 * (size_t)n_reads;          // 0xFFFFFFFF - undecided killers (min = most)
    uint32_t* up = ctx->d_death[1].p;
    // (the first lower bound - everybody's first killer - was taken by the classify kernel; the
    // upper bounds are all "never" in the first round, which is told so instead of reading them, and
    // written in full before the second)
    bool first_round = true;
    if (comm && comm->all_reduce_u32(lo, n_reads, ReduceOp::kMin, s) != 0) return comm_fail("all-reduce of the containment bounds");
    ctx->tm.death_rounds = 0;
    int cur = 0;
    bool gathered = comm == nullptr;                             // the killer lists are complete on this rank
    // Once few killers are left a round costs what the host's look at the counter costs.  A round
    // over an empty list changes nothing, so the host then enqueues several rounds at a time and
    // looks once; the list sizes of the rounds it did not look at are logged on the device (for
    // the round count) and read with the next results.
    constexpr uint32_t kFewKillers = 1u << 16, kRoundsPerLook = 5, kLogged = 64;
    constexpr uint32_t kNotSeen = 0xFFFFFFFFu;
    HIPCHECK(ctx->d_round_log.ensure(kLogged));
    std::vector<uint32_t> list_size;                             // after every round; kNotSeen = in the log
    // (one GPU: two rounds without a look from the host - C3: 1.09 M undecided after the first, 11 k after the
    // second - and what is left is finished on the device (fixed_point_kernels.hip: one workgroup with the bounds
    // in LDS, or a few resident workgroups for a long list): no more launches per round, no looks.  Before: six
    // more rounds of four launches, three looks.)
    const bool blind = comm == nullptr && ctx->use_round_batches;
    uint32_t unseen = blind ? 1u : 0u, n_logged = 0;
    constexpr uint32_t kFinishAtMost = 1u << 20;
    bool finished_on_device = false;
    uint64_t at_most = ~0ull;                                    // what the host knows of the current list's length
    for (;;) {
        if (next_count < kCountRing) {
            klist[cur ^ 1].count = ctx->d_kill_count.p + next_count++;
        } else {
            klist[cur ^ 1].count = ctx->d_kill_count.p + kCountRing + (cur ^ 1);
            HIPCHECK(hipMemsetAsync(klist[cur ^ 1].count, 0, 4, s));
        }
        launch_death_decide(klist[cur], lo, first_round ? nullptr : up, sure, klist[cur ^ 1], s, at_most);
        first_round = false;
        cur ^= 1;
        auto finish_on_device = [&]() -> int {
            // what is still undecided against sure[] as the deaths decided for good; up[], lo[] are free now
            HIPCHECK(ctx->d_death[0].ensure(n_reads));
            HIPCHECK(ctx->d_t_work[0].ensure(n_reads));
            uint32_t* const work[4] = {up, lo, ctx->d_death[0].p, ctx->d_t_work[0].p};
            const FixedPointList rest = {klist[cur].ovl, klist[cur].target, klist[cur].keeper, klist[cur].count, ctx->debug_fp_lds_limit, ctx->debug_fp_give_up};
            HIPCHECK(launch_fixed_point_finish(rest, sure, ctx->d_fp_map.p, ctx->d_fp_pack.p, work, ctx->d_counts.p + kPass2Sync,
                                               ctx->d_counts.p + kPass2Verdict, ctx->d_counts.p + kPass2FinishRounds, s));
            finished_on_device = true;
            return (int)RALA_HIP_OK;
        };
        if (blind && list_size.size() == 1) {                   // the second round is done
            list_size.push_back(kNotSeen);
            const int rc = finish_on_device();
            if (rc != RALA_HIP_OK) return rc;
            break;
        }
        // tighter bounds for the next round: up = sure, lo = min(sure, undecided killers)
        uint32_t undecided = 0;
        if (gathered && unseen && n_logged < kLogged) {
            --unseen;
            list_size.push_back(kNotSeen);
            launch_death_tighten(sure, up, lo, n_reads, s, klist[cur].count, ctx->d_round_log.p + n_logged++);
            launch_death_lower(klist[cur], lo, s, at_most);
            continue;
        }
        if (gathered) {
            HIPCHECK(d2h_small(ctx, &undecided, klist[cur].count, 4, s));
            HIPCHECK(stream_sync(ctx, s));
        } else {
            HIPCHECK(hipMemcpyAsync(lo, sure, dbytes, hipMemcpyDeviceToDevice, s));
            launch_death_lower(klist[cur], lo, s);
            launch_death_status(klist[cur].count, status, s);
            if (comm->all_reduce_u32(sure, 2 * (size_t)n_reads + 1, ReduceOp::kMin, s) != 0) return comm_fail("all-reduce of the containment bounds");
            uint32_t st = 0;
            HIPCHECK(d2h_small(ctx, &st, status, 4, s));
            HIPCHECK(stream_sync(ctx, s));
            undecided = 0xFFFFFFFFu - st;                        // the largest list of any rank
        }
        list_size.push_back(undecided);
        if (trace_on()) fprintf(stderr, "[trace] containment round %d: %u undecided\n", (int)list_size.size(), undecided);
        if (undecided == 0) break;
        if (list_size.size() > 100000) return fail(ctx, RALA_HIP_EDEVICE, "containment fixed point did not converge");
        if (!gathered) HIPCHECK(hipMemcpyAsync(up, sure, dbytes, hipMemcpyDeviceToDevice, s));
        if (gathered && ctx->use_round_batches && undecided <= kFinishAtMost) {
            // (sharded run: the ranks hold the same gathered list and the same bounds)
            const int rc = finish_on_device();
            if (rc != RALA_HIP_OK) return rc;
            break;
        }
        if (gathered) {
            at_most = undecided;                                // the lists only shrink from here
            launch_death_tighten(sure, up, lo, n_reads, s);
            launch_death_lower(klist[cur], lo, s, at_most);
            if (undecided <= kFewKillers && ctx->use_round_batches) unseen = kRoundsPerLook;
        } else if ((uint64_t)undecided * comm->world() <= (1u << 16)) {
            // few killers left: every rank takes all of them and the rest needs no collective.  `undecided` is the longest
            // list of any rank, known everywhere: every rank pads its list to that length with inert entries and blocks of one
            // size are gathered - no exchange of the lists' lengths, no look from the host (rounds 2 - 4: a count to the host,
            // a host exchange, three gathers of different lengths, a count back to the device and a wait for it)
            const uint32_t each = undecided;
            const uint64_t total = (uint64_t)each * comm->world();
            if (total > kill_room) return fail(ctx, RALA_HIP_EDEVICE, "more undecided killers than there is room for");   // (cannot happen: <= 65536)
            HIPCHECK(ctx->d_gather[0].ensure((size_t)each * 12 + 16));
            HIPCHECK(ctx->d_gather[1].ensure((size_t)total * 12 + 16));
            launch_pack_killers(klist[cur].ovl, klist[cur].target, klist[cur].keeper, klist[cur].count, each, (uint32_t*)ctx->d_gather[0].p, s);
            if (comm->all_gather(ctx->d_gather[0].p, ctx->d_gather[1].p, (size_t)each * 12, s) != 0) return comm_fail("all-gather of the undecided killers");
            launch_unpack_killers((const uint32_t*)ctx->d_gather[1].p, comm->world(), each, klist[cur ^ 1].ovl, klist[cur ^ 1].target,
                                  klist[cur ^ 1].keeper, klist[cur ^ 1].count, s);
            cur ^= 1;
            gathered = true;
            at_most = total;
        }
    }
    uint32_t* death = sure;
    HIPCHECK(hipEventRecord(ctx->ev[kEvPass2Decided], s));

    // ---- liveness, hill counters, survivors ----
    const uint32_t n_chunks = pass2_chunks(N);
    const size_t mask_words = (size_t)((N + 63) / 64);
    HIPCHECK(ctx->d_cls.ensure(2 * 8 * mask_words + 16));
    uint64_t* mask_ov = (uint64_t*)ctx->d_cls.p;
    uint64_t* mask_in = mask_ov + mask_words;
    HIPCHECK(ctx->d_fate.ensure(n_reads));
    launch_apply_death(death, ctx->d_alive.p, ctx->d_n_hills.p, ctx->d_fate.p, n_reads, ctx->d_counts.p + kPass2ReadsAlive, s);
    launch_survivor_masks(ctx->ovl, n_reads, ctx->d_valid.p, ctx->d_fate.p, death, ctx->d_crec.p, small_rec, ctx->d_rec.p,
                          ctx->d_pool.p, mask_ov, mask_in, ctx->d_chunk[0].p, ctx->d_chunk[1].p, s);
    if (comm && ctx->pool_used) {
        // Pile::check_chimeric_hills counters (pile.cpp:457-469): every slice counted its own overlaps
        HIPCHECK(ctx->d_t_tmp[0].ensure(std::max<size_t>(ctx->pool_used, n_reads) + 2));
        HIPCHECK(hipMemsetAsync(ctx->d_t_tmp[0].p, 0, (size_t)ctx->pool_used * 4, s));
        launch_hill_counts(rs, n_reads, ctx->d_t_tmp[0].p, 0, s);
        if (comm->all_reduce_u32(ctx->d_t_tmp[0].p, ctx->pool_used, ReduceOp::kSum, s) != 0) return comm_fail("all-reduce of the hill counters");
        launch_hill_counts(rs, n_reads, ctx->d_t_tmp[0].p, 1, s);
    }
    // the chunks' places in the two survivor lists: one scan; its sums come back with the other counts
    if (!launch_pair_offsets_pass(ctx->d_chunk[0].p, ctx->d_chunk[1].p, ctx->d_chunk[2].p, ctx->d_chunk[3].p, ctx->d_counts.p + kPass2Survivors,
                                  n_chunks, chunk_scan, s)) {
        return fail(ctx, RALA_HIP_EDEVICE, "scan space");
    }
    uint32_t round_log[64];
    if (n_logged && !finished_on_device) HIPCHECK(d2h_small(ctx, round_log, ctx->d_round_log.p, n_logged * 4, s));
    uint32_t counts8[kPass2LookWords] = {};            // (Pass2Counts, slots.h)
    HIPCHECK(d2h_small(ctx, counts8, ctx->d_counts.p, sizeof(counts8), s));
    HIPCHECK(stream_sync(ctx, s));
    const uint32_t n_surv[2] = {counts8[kPass2Survivors], counts8[kPass2Survivors + 1]};
    if (counts8[kPass2Verdict]) {
        return fail(ctx, RALA_HIP_EDEVICE, "containment fixed point did not converge");
    }
    ctx->t_n_alive = counts8[kPass2ReadsAlive];        // the reads that survived the second pass (the tail's rank space)
    if (finished_on_device) {
        ctx->tm.death_rounds = (uint32_t)list_size.size() + counts8[kPass2FinishRounds];
    } else {
        // rounds until the list was empty
        uint32_t at = 0;
        ctx->tm.death_rounds = (uint32_t)list_size.size();
        for (size_t r = 0; r < list_size.size(); ++r) {
            const uint32_t sz = list_size[r] == kNotSeen ? 0xFFFFFFFFu - round_log[at++] : list_size[r];
            if (sz == 0) { ctx->tm.death_rounds = (uint32_t)r + 1; break; }
        }
    }
    if (!comm) {
        // both survivor lists side by side in one device list: overlaps, then internals
        const uint32_t M = n_surv[0] + n_surv[1];
        ctx->t_n0 = n_surv[0]; ctx->t_n1 = n_surv[1];
        for (int f = 0; f < 8; ++f) HIPCHECK(ctx->d_surv_u32[f].ensure(M));
        for (int f = 0; f < 2; ++f) HIPCHECK(ctx->d_surv_u8[f].ensure(M));
        // trim in the gather re-derives the coordinates against the pass-1 piles
        if (M) launch_gather_survivors(ctx->ovl, mask_ov, mask_in, ctx->d_crec.p, small_rec, ctx->d_chunk[2].p, ctx->d_chunk[3].p, n_surv[0], survivors_view(ctx), s);
    } else {
        // this slice's survivors as one packed block, all blocks gathered, unpacked in rank order
        const uint32_t P = comm->world();
        const uint64_t m = (uint64_t)n_surv[0] + n_surv[1];
        HIPCHECK(ctx->d_list_block[0].ensure(packed_list_bytes(m) + 16));
        if (m) launch_gather_survivors(ctx->ovl, mask_ov, mask_in, ctx->d_crec.p, small_rec, ctx->d_chunk[2].p, ctx->d_chunk[3].p, n_surv[0],
                                       packed_list_view(ctx->d_list_block[0].p, m), s);
        const uint64_t mine[2] = {n_surv[0], n_surv[1]};
        std::vector<uint64_t> all(2 * (size_t)P), bytes(P);
        if (comm->host_all_gather(mine, 2, all.data(), s) != 0) return comm_fail("survivor counts");
        ListBlocks lb;
        uint64_t tot0 = 0, tot1 = 0, off = 0;
        for (uint32_t p = 0; p < P; ++p) { tot0 += all[2 * p]; tot1 += all[2 * p + 1]; }
        if (tot0 + tot1 >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "too many surviving overlaps");
        uint64_t at0 = 0, at1 = tot0;
        for (uint32_t p = 0; p < P; ++p) {
            const uint64_t mp = all[2 * p] + all[2 * p + 1];
            bytes[p] = packed_list_bytes(mp);
            lb.block_off[p] = off; lb.n0[p] = (uint32_t)all[2 * p]; lb.n1[p] = (uint32_t)all[2 * p + 1];
            lb.dst0[p] = (uint32_t)at0; lb.dst1[p] = (uint32_t)at1;
            off += bytes[p]; at0 += all[2 * p]; at1 += all[2 * p + 1];
        }
        lb.world = P;
        HIPCHECK(ctx->d_list_block[1].ensure(off + 16));
        const uint32_t M = (uint32_t)(tot0 + tot1);
        ctx->t_n0 = (uint32_t)tot0; ctx->t_n1 = (uint32_t)tot1;
        for (int f = 0; f < 8; ++f) HIPCHECK(ctx->d_surv_u32[f].ensure(M));
        for (int f = 0; f < 2; ++f) HIPCHECK(ctx->d_surv_u8[f].ensure(M));
        // The blocks travel on the side stream, beside the first kernels of the tail (list states, ranks of the reads that
        // are left, the breaks over hills: nothing of that looks at an item); gpu_tail_part_a joins in front of its first
        // kernel over the items.
        hipStream_t gs = ctx->use_side_stream ? ctx->side : s;
        if (gs != s) {
            HIPCHECK(hipEventRecord(ctx->ev[kEvGatherFork], s));
            HIPCHECK(hipStreamWaitEvent(gs, ctx->ev[kEvGatherFork], 0));
        }
        if (comm->all_gather_v(ctx->d_list_block[0].p, ctx->d_list_block[1].p, bytes.data(), 1, gs) != 0) return comm_fail("all-gather of the survivors");
        if (M) launch_unpack_lists(ctx->d_list_block[1].p, lb, survivors_view(ctx), gs);
        if (gs != s) {
            HIPCHECK(hipEventRecord(ctx->ev[kEvGatherJoin], gs));
            ctx->lists_pending = true;
        }
    }
    HIPCHECK(hipEventRecord(ctx->ev[kEvPass2End], s));
    HIPCHECK(hipGetLastError());
    return RALA_HIP_OK;
}

// what the construct stage asks of the context, for both of its entry points (the host library and the tests match on the texts)
int check_constructible(rala_hip_ctx* ctx) {
    if (!ctx->initialized) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_initialize must succeed first");
    if (ctx->tuple_mode || !ctx->inputs_set) return fail(ctx, RALA_HIP_EINVAL, "construct needs the overlaps (rala_hip_set_overlaps)");
    if (ctx->constructed) return fail(ctx, RALA_HIP_EINVAL, "object already constructed");
    return RALA_HIP_OK;
}

// pass 2's event times into ctx->tm (once the stream has passed kEvPass2End)
int pass2_times(rala_hip_ctx* ctx) {
    HIPCHECK(hipEventElapsedTime(&ctx->tm.classify_ms, ctx->ev[kEvPass2Begin], ctx->ev[kEvPass2Classified]));
    HIPCHECK(hipEventElapsedTime(&ctx->tm.death_ms, ctx->ev[kEvPass2Classified], ctx->ev[kEvPass2Decided]));
    HIPCHECK(hipEventElapsedTime(&ctx->tm.finish_ms, ctx->ev[kEvPass2Decided], ctx->ev[kEvPass2End]));
    return RALA_HIP_OK;
}

}  // namespace

// ---- stage entry points shared with the sharded runner (stages.h) ---------------------------------
int rala_hip::construct_stages(rala_hip_ctx* ctx, Comm* comm, bool sensitive_pass_follows) {
    if (!ctx) return RALA_HIP_EINVAL;
    int rc = check_constructible(ctx);
    if (rc != RALA_HIP_OK) return rc;
    construct_begun(ctx);
    HIPCHECK(hipSetDevice(ctx->device));
    rc = pass2(ctx, comm);
    if (rc != RALA_HIP_OK) return rc;
    tail_begun(ctx);
    const double t0 = now_ms();
    rc = sensitive_pass_follows ? gpu_tail_part_a(ctx) : gpu_tail_run(ctx);      // (repeats_stage builds the graph)
    if (rc != RALA_HIP_OK) return rc;
    rc = pass2_times(ctx);
    if (rc != RALA_HIP_OK) return rc;
    ctx->tm.tail_host_ms = (float)(now_ms() - t0);
    constructed(ctx);
    return RALA_HIP_OK;
}

extern "C" {

int rala_hip_construct(rala_hip_ctx* ctx, const rala_hip_overlaps* sens, uint64_t n_sens) {
    if (!ctx) return RALA_HIP_EINVAL;
    // (the state first, as construct_stages asks again: which error a caller gets does not depend on its sensitive overlaps)
    int rc = check_constructible(ctx);
    if (rc != RALA_HIP_OK) return rc;
    const bool with_sens = sens != nullptr && n_sens != 0;
    if (with_sens && !ctx->piles_resident) return fail(ctx, RALA_HIP_EINVAL, "the sensitive pass needs the piles on this context");
    if (with_sens && ctx->rowless && ctx->sens_csr_ready) {
        return fail(ctx, RALA_HIP_EINVAL, "pile_rows = 0: one sensitive construct per rala_hip_initialize (its bounds are what the rows are rebuilt from)");
    }
    HIPCHECK(hipSetDevice(ctx->device));
    rc = flush_upload(ctx);
    if (rc != RALA_HIP_OK) return rc;
    if (ctx->use_gpu_tail) {
        rc = construct_stages(ctx, nullptr, with_sens);
        if (rc != RALA_HIP_OK || !with_sens) return rc;
        // Graph::preprocess(sensitive overlaps) (graph.cpp:882-1054) works on the lists the chimera stage leaves on the
        // device: repeats annotated, the graph built from what is left
        rc = repeats_stage(ctx, ctx, nullptr, sens, n_sens);
        if (rc != RALA_HIP_OK) construct_failed(ctx);
        return rc;
    }
    // ---- the cross-check path (use_gpu_tail = 0): pass 2, then the tail on the host ----
    construct_begun(ctx);
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    rc = pass2(ctx, nullptr);
    if (rc != RALA_HIP_OK) return rc;
    const uint32_t M = ctx->t_n0 + ctx->t_n1;
    const uint32_t n_surv[2] = {ctx->t_n0, ctx->t_n1};
    tail_begun(ctx);
    // lists to the host
    std::vector<HostOvl>* lists[2] = {&ctx->overlaps, &ctx->internals};
    uint32_t* c32[8];
    for (int f = 0; f < 8; ++f) {
        HIPCHECK(ctx->p_surv_u32[f].ensure(M));
        c32[f] = ctx->p_surv_u32[f].p;
        if (M) HIPCHECK(hipMemcpyAsync(ctx->p_surv_u32[f].p, ctx->d_surv_u32[f].p, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    }
    for (int f = 0; f < 2; ++f) {
        HIPCHECK(ctx->p_surv_u8[f].ensure(M));
        if (M) HIPCHECK(hipMemcpyAsync(ctx->p_surv_u8[f].p, ctx->d_surv_u8[f].p, M, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(stream_sync(ctx, s));
    const Survivors sv = survivors_of(c32, ctx->p_surv_u8[0].p, ctx->p_surv_u8[1].p);
    for (int k = 0; k < 2; ++k) {
        const uint32_t m = n_surv[k];
        const uint32_t off = k == 0 ? 0 : n_surv[0];
        lists[k]->clear();
        // promoted internals are appended to the overlaps later: room for them up front
        lists[k]->reserve(k == 0 ? (size_t)M : (size_t)m);
        lists[k]->resize(m);
        std::vector<HostOvl>& dst = *lists[k];
        ctx->pool->chunks(m, [&](unsigned, size_t b0, size_t e0) {
            for (size_t i = b0; i < e0; ++i) dst[i] = host_item(sv, off + i);
        });
    }
    // refreshed read state: liveness after the scan, hill counters in the pool
    rc = download_read_state(ctx);
    if (rc != RALA_HIP_OK) return rc;
    rc = pass2_times(ctx);
    if (rc != RALA_HIP_OK) return rc;

    const double t0 = now_ms();
    Trace trc;
    {
        const int rc4 = preprocess_chimeras(ctx);
        if (rc4 != RALA_HIP_OK) return rc4;
    }
    if (with_sens) {
        const double t1 = now_ms();
        const int rc3 = preprocess_repeats(ctx, ctx, nullptr, sens, n_sens, false);
        if (rc3 != RALA_HIP_OK) return rc3;
        ctx->tm.repeats_ms = (float)(now_ms() - t1);
    }
    trc("preprocess total");
    build_graph(ctx);
    trc("build_graph", ctx->e_src.size());
    ctx->tm.tail_host_ms = (float)(now_ms() - t0);

    // push the final valid regions / liveness back, re-zero the piles outside them
    HIPCHECK(hipMemcpyAsync(ctx->d_begin.p, ctx->h_begin.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_end.p, ctx->h_end.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_alive.p, ctx->h_alive.data(), (size_t)n_reads, hipMemcpyHostToDevice, s));
    HIPCHECK(stream_sync(ctx, s));
    constructed(ctx);
    return RALA_HIP_OK;
}

}  // extern "C"
