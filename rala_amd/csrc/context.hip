// librala_hip: the front of the C ABI (include/rala_hip.h) - a context made and destroyed, its options, its inputs (reads;
// overlaps, or bounds as tuples, records or a sharded run's blocks), per-read state installed from outside and handed out.
// Host code around copies: no kernel of the hot path is launched here.  What these calls mean for the context's life is in
// lifecycle.h; the stages are in initialize.hip, construct.hip, sensitive.hip and transitive.hip, the getters in getters.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>

#include "ctx_check.h"
#include "lifecycle.h"
#include "scan_pass.h"
#include "slots.h"
#include "stages.h"

using namespace rala_hip;

namespace {

// What the three setters of bound inputs end with (they began with inputs_withdrawn), their own pointers and counts in
// place: n_events bound events in all (one per tuple, two per record) - room for them and for the scans over them - then
// the transition.
int bound_inputs_adopted(rala_hip_ctx* ctx, Inputs kind, uint64_t n_events) {
    HIPCHECK(ctx->d_ev.ensure(n_events + 8));
    HIPCHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(std::max<uint64_t>(n_events, ctx->n_reads) + 2)));
    ctx->n_tuples = n_events;           // (what the tuple paths see, whatever the kind)
    inputs_adopted(ctx, kind);
    return RALA_HIP_OK;
}

// an installed state with more intervals than the pool holds: a pool of that size (and a little more)
int grow_pool_to(rala_hip_ctx* ctx, uint64_t pool_count) {
    if (pool_count <= ctx->pool_cap) return RALA_HIP_OK;
    ctx->pool_cap = (uint32_t)pool_count + 1024;
    HIPCHECK(ctx->d_pool.ensure(ctx->pool_cap));
    return RALA_HIP_OK;
}

// What installing per-read state that lies in the device arrays ends with (install_read_state, rala_hip_import_state_device):
// the last run's timings and lists are gone, the pool's counter is the installed one, the filtered reads are counted where
// they lie (the host's vectors are fetched by the first getter), the transition, and the verdict on a state without live reads.
int finish_install(rala_hip_ctx* ctx, uint64_t pool_count, bool valid_ready) {
    hipStream_t s = ctx->stream;
    ctx->tm = rala_hip_timings();
    ctx->overlaps.clear(); ctx->internals.clear();
    uint32_t small[kInstallSmallWords] = {};
    small[kSmallPoolCount] = (uint32_t)pool_count;
    HIPCHECK(hipMemcpyAsync(ctx->d_small.p, small, sizeof(small), hipMemcpyHostToDevice, s));
    HIPCHECK(ctx->d_cc_flags.ensure(kCcFlagsWords));
    HIPCHECK(hipMemsetAsync(ctx->d_cc_flags.p + kCcInstallDead, 0, 4, s));
    launch_count_zero_u8(ctx->d_alive.p, (uint32_t)ctx->n_reads, ctx->d_cc_flags.p + kCcInstallDead, s);
    uint32_t n_dead = 0;
    HIPCHECK(d2h_small(ctx, &n_dead, ctx->d_cc_flags.p + kCcInstallDead, 4, s));
    HIPCHECK(stream_sync(ctx, s));                  // `small` is a local
    results_dropped(ctx);
    state_installed(ctx, n_dead, (uint32_t)pool_count, false, false, valid_ready);
    if (n_dead == ctx->n_reads) return fail(ctx, RALA_HIP_EFILTERED, "filtered all sequences");
    return RALA_HIP_OK;
}

}  // namespace

// Small device -> host reads (counters, flags) go through a pinned staging area: an async copy
// into pageable memory is staged by the runtime and costs tens of microseconds more, and the
// tail does a dozen of them per call.  d2h_small queues the copy, stream_sync waits for the
// stream and delivers what was queued.
hipError_t rala_hip::d2h_small(rala_hip_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (ctx->p_stage.ensure(256) != hipSuccess || ctx->stage_used + bytes > 256 * sizeof(uint32_t) ||
        ctx->stage_pending.size() >= 16) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    }
    char* at = (char*)ctx->p_stage.p + ctx->stage_used;
    const hipError_t e = hipMemcpyAsync(at, src, bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    ctx->stage_pending.push_back({dst, ctx->stage_used, bytes});
    ctx->stage_used += (bytes + 7) & ~(size_t)7;
    return hipSuccess;
}

hipError_t rala_hip::stream_sync(rala_hip_ctx* ctx, hipStream_t s) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) {      // a failed wait delivers nothing
        for (const auto& c : ctx->stage_pending) memcpy(c.dst, (const char*)ctx->p_stage.p + c.offset, c.bytes);
    }
    ctx->stage_pending.clear();
    ctx->stage_used = 0;
    return e;
}

// RALA_HIP_MEM_HOST_ASYNC columns that rala_hip_initialize has not uploaded yet: now, for a caller that reads them first
int rala_hip::flush_upload(rala_hip_ctx* ctx) {
    if (!ctx->upload_pending) return RALA_HIP_OK;
    for (int k = 0; k < 7; ++k) HIPCHECK(hipMemcpy(ctx->d_ovl_u32[k].p, ctx->up_src[k], (size_t)ctx->n_ovl * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_ovl_strand.p, ctx->up_strand, ctx->n_ovl, hipMemcpyHostToDevice));
    upload_done(ctx);
    return RALA_HIP_OK;
}

// An owner of a sharded run: its input is the blocks of all senders where they lie (base: what was received; base_self:
// the send buffer, for the rank's own block); n_records of them in all.  rala_hip_initialize takes it from there.
int rala_hip::set_bound_blocks(rala_hip_ctx* ctx, const uint64_t* base, const uint64_t* base_self, const ShardBlocks& blocks,
                               const ShardGeometry& g, uint64_t n_records) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (n_records >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_EINVAL, "too many records");
    HIPCHECK(hipSetDevice(ctx->device));
    inputs_withdrawn(ctx);
    ctx->blocks_base = base; ctx->blocks_base_self = base_self; ctx->blocks = blocks; ctx->shard_geom = g;
    ctx->n_block_records = n_records;
    return bound_inputs_adopted(ctx, Inputs::kBlocks, 2 * n_records);
}

int rala_hip::install_read_state(rala_hip_ctx* ctx, uint64_t pool_count) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (ctx->n_ovl && !ctx->valid_ready) return fail(ctx, RALA_HIP_EINVAL, "validity bits required (rala_hip_dedupe)");
    if (pool_count > ctx->pool_cap) return fail(ctx, RALA_HIP_ECAPACITY, "interval pool smaller than the installed state");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcu = flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    return finish_install(ctx, pool_count, ctx->valid_ready);
}

extern "C" {

int rala_hip_create(int device, rala_hip_ctx** out) {
    if (!out) return RALA_HIP_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return RALA_HIP_EDEVICE;
    if (hipSetDevice(device) != hipSuccess) return RALA_HIP_EDEVICE;
    rala_hip_ctx* ctx = new rala_hip_ctx;
    ctx->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
            ctx->n_compute_units = (uint32_t)prop.multiProcessorCount;
        }
    }
    // (the side stream at the highest priority the device offers: what runs there beside a kernel that fills the chip - the
    // position-space kernels of the sensitive pass, whose workgroups want most of a compute unit's LDS - gets the compute
    // units as they come free instead of when the other kernel has drained)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    bool ok = hipStreamCreate(&ctx->stream) == hipSuccess &&
              hipStreamCreateWithPriority(&ctx->side, hipStreamDefault, prio_greatest) == hipSuccess &&
              hipStreamCreate(&ctx->aux) == hipSuccess;
    for (auto& e : ctx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    static_assert(sizeof(ctx->ev) / sizeof(ctx->ev[0]) == kEvCount, "one event per name of slots.h");
    ok = ok && ctx->d_small.ensure(kSmallWords) == hipSuccess;
    if (!ok) {                                  // (rala_hip_destroy releases whatever was created)
        rala_hip_destroy(ctx);
        return RALA_HIP_EDEVICE;
    }
    ctx->pool.reset(new HostPool(std::min(16u, std::max(1u, std::thread::hardware_concurrency()))));
    *out = ctx;
    return RALA_HIP_OK;
}

void rala_hip_destroy(rala_hip_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    ctx->stage_pending.clear();             // nobody is waiting for staged copies any more
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
    for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev_up) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev_layout) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev_names) if (e) (void)hipEventDestroy(e);
    if (ctx->copy) (void)hipStreamDestroy(ctx->copy);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* rala_hip_last_error(const rala_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int rala_hip_set_option(rala_hip_ctx* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return RALA_HIP_EINVAL;
    if (!strcmp(key, "interval_pool_per_read_x1000")) { ctx->pool_per_read_x1000 = value; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_big_caps")) { ctx->debug_big_caps = value; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_force_big")) { ctx->debug_force_big = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "max_lds_read_len")) { ctx->max_lds_read_len = value; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_pile_stop_after")) { ctx->debug_pile_stop_after = value; return RALA_HIP_OK; }
    if (!strcmp(key, "use_run_kernel")) { ctx->use_run_kernel = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_round_batches")) { ctx->use_round_batches = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_bound_records")) { ctx->use_bound_records = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_fused_emit")) { ctx->use_fused_emit = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "ingest_window_bytes")) { ctx->ingest_window_bytes = std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_sequence_window")) { ctx->debug_sequence_window = std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "gzip_on_device")) { ctx->gzip_on_device = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "gzip_members")) { ctx->gzip_members = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "gzip_in_pieces")) { ctx->gzip_in_pieces = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "bgzf_in_pieces")) { ctx->bgzf_in_pieces = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "gzip_chunk_bytes")) { ctx->gzip_chunk_bytes = value > 0 ? value : 64 << 10; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_gzip_false_sync")) { ctx->debug_gzip_false_sync = (uint32_t)std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "pile_rows")) { ctx->pile_rows = value ? 1u : 0u; return RALA_HIP_OK; }
    if (!strcmp(key, "pile_rows_scratch_mb")) { ctx->pile_rows_scratch_mb = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 20)); return RALA_HIP_OK; }
    if (!strcmp(key, "keep_bases")) { ctx->keep_bases = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "spell_window_mb")) { ctx->spell_window_mb = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 20)); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_spell_window")) { ctx->debug_spell_window = std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "pile_chunk_mb")) { ctx->pile_chunk_mb = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 20)); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_ev_events")) { ctx->debug_ev_events = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_count_window")) { ctx->debug_count_window = (uint32_t)std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_part_shift")) { ctx->debug_part_shift = (uint32_t)std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_dedupe_list_cap")) { ctx->debug_dedupe_list_cap = (uint32_t)std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_fp_lds_limit")) { ctx->debug_fp_lds_limit = (uint32_t)std::max<int64_t>(0, value); return RALA_HIP_OK; }
    if (!strcmp(key, "debug_fp_give_up")) { ctx->debug_fp_give_up = value == 2 ? 2u : value != 0 ? 1u : 0u; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_chunk_fail")) { ctx->debug_chunk_fail = value; return RALA_HIP_OK; }
    if (!strcmp(key, "debug_fail_construct")) { ctx->debug_fail_construct = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_gpu_tail")) { ctx->use_gpu_tail = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_fixed_buckets")) { ctx->use_fixed_buckets = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_partitioned_buckets")) { ctx->use_partitioned_buckets = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "use_side_stream")) { ctx->use_side_stream = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "sensitive_in_device_memory")) { ctx->sens_in_device = value != 0; return RALA_HIP_OK; }
    if (!strcmp(key, "layout_fused_max")) {
        if (value < 0 || value > 1024) return fail(ctx, RALA_HIP_EINVAL, "layout_fused_max: 0 .. 1024");
        ctx->layout_fused_max = value;
        return RALA_HIP_OK;
    }
    if (!strcmp(key, "host_threads")) {
        ctx->host_threads = value;
        ctx->pool.reset(new HostPool((unsigned)std::max<int64_t>(1, std::min<int64_t>(value, 256))));
        return RALA_HIP_OK;
    }
    return fail(ctx, RALA_HIP_EINVAL, "unknown option");
}

void* rala_hip_stream(rala_hip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int rala_hip_set_reads(rala_hip_ctx* ctx, const uint32_t* read_len, uint64_t n_reads) {
    if (!ctx || (!read_len && n_reads)) return RALA_HIP_EINVAL;
    if (n_reads >= 0x7FFFFFFFull) return fail(ctx, RALA_HIP_EINVAL, "too many reads");
    HIPCHECK(hipSetDevice(ctx->device));
    HIPCHECK(hipStreamSynchronize(ctx->side));
    HIPCHECK(hipStreamSynchronize(ctx->aux));
    ctx->n_reads = n_reads;
    ctx->h_read_len.assign(read_len, read_len + n_reads);
    ctx->max_read_len = 0;
    for (uint64_t r = 0; r < n_reads; ++r) ctx->max_read_len = std::max(ctx->max_read_len, read_len[r]);
    {
        // length classes of the pile chain (kernels.h: kPileClassBases)
        uint32_t cnt[kPileClasses] = {};
        auto cls = [](uint32_t n) {
            uint32_t c = 0;
            while (c + 1 < kPileClasses && n > kPileClassBases[c]) ++c;
            return c;
        };
        for (uint64_t r = 0; r < n_reads; ++r) ++cnt[cls(read_len[r])];
        for (uint32_t c = 0; c < kPileClasses; ++c) ctx->n_class[c] = cnt[c];
        if (cnt[0] != n_reads) {
            std::vector<uint32_t> order(n_reads);
            uint32_t at[kPileClasses] = {};
            for (uint32_t c = 1; c < kPileClasses; ++c) at[c] = at[c - 1] + cnt[c - 1];
            for (uint64_t r = 0; r < n_reads; ++r) order[at[cls(read_len[r])]++] = (uint32_t)r;
            HIPCHECK(ctx->d_class_order.ensure(n_reads));
            HIPCHECK(hipMemcpy(ctx->d_class_order.p, order.data(), n_reads * 4, hipMemcpyHostToDevice));
        }
    }
    ctx->h_pile_off.resize(n_reads + 1);
    // Rows start on 128-byte boundaries (64 elements): a row's first and last cache line are then its own, not shared
    // with the neighbouring rows, which other wavefronts write at other times.  Round 4, one box, pile kernel at C3:
    // 16-byte boundaries (rounds 1 - 3: what the 16-byte stores need) 4.26 ms, 128 bytes 4.17, 1 KB 4.18, 4 KB 4.21
    // (round 4, r4_rowalign.sh under docs/history).
    constexpr uint64_t row_align = 64;
    uint64_t off = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        ctx->h_pile_off[r] = off;
        off += ((uint64_t)read_len[r] + row_align - 1) & ~(row_align - 1);
    }
    ctx->h_pile_off[n_reads] = off;
    ctx->pile_elems = off;
    HIPCHECK(ctx->d_read_len.ensure(n_reads + 1));
    HIPCHECK(ctx->d_pile_off.ensure(n_reads + 1));
    ctx->d_pile.release();                       // allocated by rala_hip_initialize (owners only)
    HIPCHECK(hipMemcpy(ctx->d_read_len.p, read_len, n_reads * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_pile_off.p, ctx->h_pile_off.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice));
    HIPCHECK(ctx->d_order.ensure(n_reads + 1));
    HIPCHECK(ctx->d_overflow.ensure(n_reads + 1));
    HIPCHECK(ctx->d_ev_off.ensure(n_reads + 2)); HIPCHECK(ctx->d_cursor.ensure(n_reads + 2));
    HIPCHECK(ctx->d_suspect.ensure(n_reads + 1));
    HIPCHECK(ctx->d_begin.ensure(n_reads)); HIPCHECK(ctx->d_end.ensure(n_reads));
    HIPCHECK(ctx->d_median.ensure(n_reads)); HIPCHECK(ctx->d_p10.ensure(n_reads));
    HIPCHECK(ctx->d_alive.ensure(n_reads)); HIPCHECK(ctx->d_n_pits.ensure(n_reads));
    HIPCHECK(ctx->d_n_hills.ensure(n_reads)); HIPCHECK(ctx->d_iv_slot.ensure(n_reads));
    HIPCHECK(ctx->d_death[0].ensure(n_reads)); HIPCHECK(ctx->d_death[1].ensure(n_reads));
    // scans run over reads as well as over overlaps / tuples, whichever call comes first
    HIPCHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(std::max<uint64_t>(std::max(ctx->n_ovl, ctx->n_tuples), n_reads) + 2)));
    // host mirrors of the per-read state.  They are NOT registered with the runtime: registration
    // pins whole pages, small vectors of different contexts share pages of the heap, and
    // unregistering one context's vectors then unmapped pages another context's copies still went
    // to ("Memory access fault by GPU" in a later, unrelated call).
    ctx->h_begin.resize(n_reads); ctx->h_end.resize(n_reads); ctx->h_median.resize(n_reads);
    ctx->h_p10.resize(n_reads); ctx->h_alive.resize(n_reads); ctx->h_n_pits.resize(n_reads);
    ctx->h_n_hills.resize(n_reads); ctx->h_slot.resize(n_reads);
    // (a hint: a pool that turns out too small grows to the counted need; 0 = start at 16 slots, for the tests of that)
    ctx->pool_cap = (uint32_t)std::max<int64_t>(ctx->pool_per_read_x1000 == 0 ? 16 : 1024, (int64_t)n_reads * ctx->pool_per_read_x1000 / 1000);
    ctx->pool_cap_first = ctx->pool_cap;        // (the repeat hills' pool starts there too, and grows on its own)
    ctx->rep_pool_cap = 0;
    HIPCHECK(ctx->d_pool.ensure(ctx->pool_cap));
    results_dropped(ctx);
    return RALA_HIP_OK;
}

int rala_hip_set_overlaps(rala_hip_ctx* ctx, const rala_hip_overlaps* o, uint64_t n, int mem) {
    if (!ctx || (!o && n)) return RALA_HIP_EINVAL;
    // (2 n bound pairs in 32 bits - the partitioned bucketing's offsets, kernels.h: kBucketPairShift; the other bucketing paths count
    // 4 n events and say so in rala_hip_initialize when they meet more)
    if (n >= 0xFFFFFFF0ull / 2) return fail(ctx, RALA_HIP_EINVAL, "too many overlaps for 32-bit bound offsets");
    HIPCHECK(hipSetDevice(ctx->device));
    HIPCHECK(hipStreamSynchronize(ctx->side));          // a failed call may have left work there
    HIPCHECK(hipStreamSynchronize(ctx->aux));
    if (ctx->copy) HIPCHECK(hipStreamSynchronize(ctx->copy));
    inputs_withdrawn(ctx);              // (whatever fails below: no inputs, no results, until inputs_adopted)
    upload_done(ctx);
    if (mem == RALA_HIP_MEM_HOST_ASYNC && !ctx->copy) {
        // (made when first asked for: a process has few hardware queues - four by default - and its streams share them; a
        // stream that is not used must not push a context's main and aux streams onto one queue.  It did, in the sharded
        // runner's owner contexts: their small pile kernels ran in front of the big one instead of beside it, +0.13 ms at C3)
        // (all or nothing: a stream whose events could not all be made would leave later calls with null events - advisor round 5)
        hipStream_t made = nullptr;
        HIPCHECK(hipStreamCreate(&made));
        hipError_t bad = hipSuccess;
        for (auto& e : ctx->ev_up) {
            e = nullptr;
            if (bad == hipSuccess) bad = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        }
        if (bad != hipSuccess) {
            for (auto& e : ctx->ev_up) { if (e) (void)hipEventDestroy(e); e = nullptr; }
            (void)hipStreamDestroy(made);
            HIPCHECK(bad);
        }
        ctx->copy = made;
    }
    const uint32_t* src[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (n) {
        src[0] = o->a_id; src[1] = o->b_id; src[2] = o->a_begin; src[3] = o->a_end;
        src[4] = o->b_begin; src[5] = o->b_end; src[6] = o->length;
    }
    const uint32_t* dev[7];
    const uint8_t* dev_strand;
    if (mem == RALA_HIP_MEM_DEVICE) {
        for (int k = 0; k < 7; ++k) dev[k] = src[k];
        dev_strand = n ? o->strand : nullptr;
    } else {
        // (RALA_HIP_MEM_HOST_ASYNC: room now, the copies in rala_hip_initialize - upload_columns)
        const bool later = mem == RALA_HIP_MEM_HOST_ASYNC && n != 0;
        for (int k = 0; k < 7; ++k) {
            HIPCHECK(ctx->d_ovl_u32[k].ensure(n));
            if (n && !later) HIPCHECK(hipMemcpy(ctx->d_ovl_u32[k].p, src[k], n * 4, hipMemcpyHostToDevice));
            dev[k] = ctx->d_ovl_u32[k].p;
            ctx->up_src[k] = src[k];
        }
        HIPCHECK(ctx->d_ovl_strand.ensure(n));
        if (n && !later) HIPCHECK(hipMemcpy(ctx->d_ovl_strand.p, o->strand, n, hipMemcpyHostToDevice));
        dev_strand = ctx->d_ovl_strand.p;
        ctx->up_strand = n ? o->strand : nullptr;
        if (later) upload_deferred(ctx);
    }
    ctx->ovl.a_id = dev[0]; ctx->ovl.b_id = dev[1]; ctx->ovl.a_begin = dev[2]; ctx->ovl.a_end = dev[3];
    ctx->ovl.b_begin = dev[4]; ctx->ovl.b_end = dev[5]; ctx->ovl.length = dev[6]; ctx->ovl.strand = dev_strand;
    ctx->ovl.n = n;
    ctx->ovl.base = 0;
    HIPCHECK(ctx->d_valid.ensure(n));
    HIPCHECK(ctx->d_ev.ensure(4 * n + 8));
    HIPCHECK(ctx->d_cls.ensure(n / 4 + 64));        // survivor masks of the second pass: two bits per overlap
    for (int k = 0; k < 4; ++k) HIPCHECK(ctx->d_chunk[k].ensure(pass2_chunks(n) + 2));
    HIPCHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(std::max<uint64_t>(n, ctx->n_reads) + 2)));
    ctx->n_ovl = n;
    inputs_adopted(ctx, Inputs::kOverlaps);
    return RALA_HIP_OK;
}

int rala_hip_get_device_state(rala_hip_ctx* ctx, rala_hip_device_state* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    if (!ctx->initialized) return fail(ctx, RALA_HIP_EINVAL, "not initialized");
    out->begin = ctx->d_begin.p; out->end = ctx->d_end.p; out->median = ctx->d_median.p; out->p10 = ctx->d_p10.p;
    out->alive = ctx->d_alive.p; out->n_pits = ctx->d_n_pits.p; out->n_hills = ctx->d_n_hills.p;
    out->slot = ctx->d_iv_slot.p; out->pool = ctx->d_pool.p; out->pool_count = (size_t)ctx->pool_used;
    out->valid = ctx->valid_ready ? ctx->d_valid.p : nullptr;
    return RALA_HIP_OK;
}

int rala_hip_copy_device_state(rala_hip_ctx* ctx, const rala_hip_device_state* dst) {
    if (!ctx || !dst) return RALA_HIP_EINVAL;
    const bool per_read = dst->begin || dst->end || dst->median || dst->p10 || dst->alive || dst->n_pits ||
                          dst->n_hills || dst->slot || dst->pool;
    if (per_read && !ctx->initialized) return fail(ctx, RALA_HIP_EINVAL, "not initialized");
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = ctx->n_reads;
    auto cp = [&](const void* to, const void* from, size_t bytes) -> hipError_t {
        if (!to || bytes == 0) return hipSuccess;
        return hipMemcpyAsync(const_cast<void*>(to), from, bytes, hipMemcpyDeviceToDevice, s);
    };
    HIPCHECK(cp(dst->begin, ctx->d_begin.p, n * 4));
    HIPCHECK(cp(dst->end, ctx->d_end.p, n * 4));
    HIPCHECK(cp(dst->median, ctx->d_median.p, n * 2));
    HIPCHECK(cp(dst->p10, ctx->d_p10.p, n * 2));
    HIPCHECK(cp(dst->alive, ctx->d_alive.p, n));
    HIPCHECK(cp(dst->n_pits, ctx->d_n_pits.p, n * 4));
    HIPCHECK(cp(dst->n_hills, ctx->d_n_hills.p, n * 4));
    HIPCHECK(cp(dst->slot, ctx->d_iv_slot.p, n * 4));
    if (dst->pool) {
        if (dst->pool_count < (size_t)ctx->pool_used) return fail(ctx, RALA_HIP_ECAPACITY, "pool buffer too small");
        HIPCHECK(cp(dst->pool, ctx->d_pool.p, (size_t)ctx->pool_used * sizeof(Interval)));
    }
    if (dst->valid) {
        if (!ctx->valid_ready) return fail(ctx, RALA_HIP_EINVAL, "no validity bits on this context");
        HIPCHECK(cp(dst->valid, ctx->d_valid.p, ctx->n_ovl));
    }
    HIPCHECK(stream_sync(ctx, s));
    return RALA_HIP_OK;
}

int rala_hip_import_state_device(rala_hip_ctx* ctx, const rala_hip_device_state* in) {
    if (!ctx || !in || !in->begin || !in->end || !in->median || !in->p10 || !in->alive || !in->n_pits ||
        !in->n_hills || !in->slot) {
        return RALA_HIP_EINVAL;
    }
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (ctx->n_ovl && !in->valid) return fail(ctx, RALA_HIP_EINVAL, "valid bits required");
    if (in->pool_count && !in->pool) return RALA_HIP_EINVAL;
    HIPCHECK(hipSetDevice(ctx->device));
    // (columns handed over with RALA_HIP_MEM_HOST_ASYNC leave inside rala_hip_initialize; a caller that installs the read state
    // instead must not find them still on the host - advisor round 5)
    { const int rcu = flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    hipStream_t s = ctx->stream;
    const uint64_t n = ctx->n_reads;
    { const int rcp = grow_pool_to(ctx, in->pool_count); if (rcp != RALA_HIP_OK) return rcp; }
    HIPCHECK(hipMemcpyAsync(ctx->d_begin.p, in->begin, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_end.p, in->end, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_median.p, in->median, n * 2, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_p10.p, in->p10, n * 2, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_alive.p, in->alive, n, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_n_pits.p, in->n_pits, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_n_hills.p, in->n_hills, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_iv_slot.p, in->slot, n * 4, hipMemcpyDeviceToDevice, s));
    if (in->pool_count) {
        HIPCHECK(hipMemcpyAsync(ctx->d_pool.p, in->pool, (size_t)in->pool_count * sizeof(Interval), hipMemcpyDeviceToDevice, s));
    }
    if (ctx->n_ovl) HIPCHECK(hipMemcpyAsync(ctx->d_valid.p, in->valid, ctx->n_ovl, hipMemcpyDeviceToDevice, s));
    return finish_install(ctx, in->pool_count, true);
}

int rala_hip_set_bound_tuples(rala_hip_ctx* ctx, const uint64_t* tuples, uint64_t n, int mem) {
    if (!ctx || (n && !tuples)) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (n >= 0xFFFFFFF0ull) return fail(ctx, RALA_HIP_EINVAL, "too many tuples");
    HIPCHECK(hipSetDevice(ctx->device));
    inputs_withdrawn(ctx);
    if (mem == RALA_HIP_MEM_DEVICE) {
        ctx->tuples = (const uint2*)tuples;
    } else {
        HIPCHECK(ctx->d_tuple.ensure(n));
        if (n) HIPCHECK(hipMemcpy(ctx->d_tuple.p, tuples, n * 8, hipMemcpyHostToDevice));
        ctx->tuples = ctx->d_tuple.p;
    }
    return bound_inputs_adopted(ctx, Inputs::kTuples, n);
}

int rala_hip_set_bound_records(rala_hip_ctx* ctx, const uint64_t* records, uint64_t n, int mem) {
    if (!ctx || (n && !records)) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (n >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_EINVAL, "too many records");
    if (!rala_hip_bound_records_fit(ctx, 1)) return fail(ctx, RALA_HIP_EINVAL, "reads too long or too many for bound records");
    HIPCHECK(hipSetDevice(ctx->device));
    inputs_withdrawn(ctx);
    if (mem == RALA_HIP_MEM_DEVICE) {
        ctx->records = records;
    } else {
        HIPCHECK(ctx->d_record.ensure(n + 8));
        if (n) HIPCHECK(hipMemcpy(ctx->d_record.p, records, n * 8, hipMemcpyHostToDevice));
        ctx->records = ctx->d_record.p;
    }
    if (!ctx->records) { HIPCHECK(ctx->d_record.ensure(8)); ctx->records = ctx->d_record.p; }   // (an empty share)
    ctx->n_records = n;
    return bound_inputs_adopted(ctx, Inputs::kRecords, 2 * n);
}

int rala_hip_import_state(rala_hip_ctx* ctx, const uint8_t* valid, const uint32_t* begin, const uint32_t* end,
                          const uint16_t* median, const uint16_t* p10, const uint8_t* alive,
                          const uint64_t* pits_off, const uint32_t* pits_pairs, const uint32_t* pits_aux,
                          const uint64_t* hills_off, const uint32_t* hills_pairs) {
    if (!ctx || !begin || !end || !median || !p10 || !alive || !pits_off || !hills_off) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (ctx->n_ovl && !valid) return fail(ctx, RALA_HIP_EINVAL, "valid bits required");
    HIPCHECK(hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_reads;
    ctx->tm = rala_hip_timings();
    ctx->overlaps.clear(); ctx->internals.clear();
    std::vector<uint32_t> np(n), nh(n);
    std::vector<uint32_t> slot(n, 0xFFFFFFFFu);
    std::vector<Interval> pool;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t a = pits_off[r + 1] - pits_off[r], b = hills_off[r + 1] - hills_off[r];
        if (a > 0xFFFFFFFFull || b > 0xFFFFFFFFull) return fail(ctx, RALA_HIP_EINVAL, "too many intervals on a read");
        np[r] = (uint32_t)a; nh[r] = (uint32_t)b;
        if (a + b == 0) continue;
        slot[r] = (uint32_t)pool.size();
        for (uint64_t k = pits_off[r]; k < pits_off[r + 1]; ++k) {
            Interval iv; iv.first = pits_pairs[2 * k]; iv.second = pits_pairs[2 * k + 1]; iv.aux = pits_aux[k];
            pool.push_back(iv);
        }
        for (uint64_t k = hills_off[r]; k < hills_off[r + 1]; ++k) {
            Interval iv; iv.first = hills_pairs[2 * k]; iv.second = hills_pairs[2 * k + 1]; iv.aux = 0;
            pool.push_back(iv);
        }
    }
    { const int rcp = grow_pool_to(ctx, pool.size()); if (rcp != RALA_HIP_OK) return rcp; }
    const uint32_t used = (uint32_t)pool.size();
    uint32_t small[kInstallSmallWords] = {};
    small[kSmallPoolCount] = used;
    HIPCHECK(hipMemcpy(ctx->d_small.p, small, sizeof(small), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_begin.p, begin, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_end.p, end, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_median.p, median, n * 2, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_p10.p, p10, n * 2, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_alive.p, alive, n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_n_pits.p, np.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_n_hills.p, nh.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_iv_slot.p, slot.data(), n * 4, hipMemcpyHostToDevice));
    if (used) HIPCHECK(hipMemcpy(ctx->d_pool.p, pool.data(), (size_t)used * sizeof(Interval), hipMemcpyHostToDevice));
    if (ctx->n_ovl) HIPCHECK(hipMemcpy(ctx->d_valid.p, valid, ctx->n_ovl, hipMemcpyHostToDevice));
    // (the state came from the host and goes back into its vectors at once: they are fresh, and the filtered reads are counted there)
    results_dropped(ctx);
    const int rc = download_read_state(ctx);
    if (rc != RALA_HIP_OK) return rc;
    uint64_t n_dead = 0;
    for (uint64_t r = 0; r < n; ++r) if (!ctx->h_alive[r]) ++n_dead;
    state_installed(ctx, n_dead, used, false, false, true);
    if (n_dead == n) return fail(ctx, RALA_HIP_EFILTERED, "filtered all sequences");
    return RALA_HIP_OK;
}

}  // extern "C"
