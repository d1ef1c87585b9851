// librala_hip: the results of a context as the host asks for them.  Implements the rala_hip_get_* calls of rala_hip.h
// (rala_hip_get_device_state and its kin are context.hip's) and download_read_state of stages.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "lifecycle.h"
#include "orchestration.h"

using namespace rala_hip;


// ---- host mirror of the per-read state -------------------------------------------
int rala_hip::download_read_state(rala_hip_ctx* ctx) {
    const uint64_t n = ctx->n_reads;
    HIPCHECK(hipSetDevice(ctx->device));        // (getters may be called with another rank's device current)
    ctx->h_begin.resize(n); ctx->h_end.resize(n); ctx->h_median.resize(n); ctx->h_p10.resize(n);
    ctx->h_alive.resize(n); ctx->h_n_pits.resize(n); ctx->h_n_hills.resize(n); ctx->h_slot.resize(n);
    hipStream_t s = ctx->stream;
    HIPCHECK(hipMemcpyAsync(ctx->h_begin.data(), ctx->d_begin.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_end.data(), ctx->d_end.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_median.data(), ctx->d_median.p, n * 2, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_p10.data(), ctx->d_p10.p, n * 2, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_alive.data(), ctx->d_alive.p, n, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_n_pits.data(), ctx->d_n_pits.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_n_hills.data(), ctx->d_n_hills.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctx->h_slot.data(), ctx->d_iv_slot.p, n * 4, hipMemcpyDeviceToHost, s));
    uint32_t pool_count = 0;
    HIPCHECK(d2h_small(ctx, &pool_count, ctx->d_small.p + kSmallPoolCount, 4, s));
    HIPCHECK(stream_sync(ctx, s));
    const uint32_t used = std::min(pool_count, ctx->pool_cap);
    ctx->pool_used = used;
    ctx->h_pool.resize(used);
    if (used) {
        HIPCHECK(hipMemcpy(ctx->h_pool.data(), ctx->d_pool.p, (size_t)used * sizeof(Interval), hipMemcpyDeviceToHost));
    }
    host_mirrors_fresh(ctx);
    return RALA_HIP_OK;
}

extern "C" {

// ---- results ---------------------------------------------------------------------------
int rala_hip_get_valid(rala_hip_ctx* ctx, uint8_t* valid) {
    if (!ctx || !valid) return RALA_HIP_EINVAL;
    if (!ctx->valid_ready) return fail(ctx, RALA_HIP_EINVAL, "run rala_hip_dedupe or rala_hip_initialize first");
    HIPCHECK(hipSetDevice(ctx->device));
    if (ctx->n_ovl) HIPCHECK(hipMemcpy(valid, ctx->d_valid.p, ctx->n_ovl, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

int rala_hip_get_piles(rala_hip_ctx* ctx, uint32_t* begin, uint32_t* end, uint16_t* median, uint16_t* p10,
                       uint8_t* alive) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!ctx->initialized) return fail(ctx, RALA_HIP_EINVAL, "not initialized");
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    const uint64_t n = ctx->n_reads;
    for (uint64_t r = 0; r < n; ++r) {
        const bool a = ctx->h_alive[r];
        if (begin) begin[r] = a ? ctx->h_begin[r] : 0;
        if (end) end[r] = a ? ctx->h_end[r] : 0;
        if (median) median[r] = a ? ctx->h_median[r] : 0;
        if (p10) p10[r] = a ? ctx->h_p10[r] : 0;
        if (alive) alive[r] = a;
    }
    return RALA_HIP_OK;
}

int rala_hip_get_pile_data(rala_hip_ctx* ctx, uint64_t read, uint16_t* data) {
    if (!ctx || !data) return RALA_HIP_EINVAL;
    if (!ctx->initialized || read >= ctx->n_reads) return fail(ctx, RALA_HIP_EINVAL, "bad read / not initialized");
    if (!ctx->piles_resident) return fail(ctx, RALA_HIP_EINVAL, "piles live on the owning rank's context");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    const uint32_t n = ctx->h_read_len[read];
    { const int rcr = pile_row_to_host(ctx, read, data); if (rcr != RALA_HIP_OK) return rcr; }
    // Pile::shrink zeroes outside the current valid region (pile.cpp:311-318); the
    // host tail narrows regions after the pile was written
    if (ctx->h_alive[read]) {
        const uint32_t B = ctx->h_begin[read], E = ctx->h_end[read];
        for (uint32_t j = 0; j < B && j < n; ++j) data[j] = 0;
        for (uint32_t j = E; j < n; ++j) data[j] = 0;
    }
    return RALA_HIP_OK;
}

int rala_hip_get_pile_rows_info(rala_hip_ctx* ctx, uint64_t* resident_bytes, uint64_t* rows_materialised) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (resident_bytes) *resident_bytes = ctx->d_pile.p ? (uint64_t)ctx->d_pile.n * sizeof(uint16_t) : 0;
    if (rows_materialised) *rows_materialised = ctx->rows_materialised;
    return RALA_HIP_OK;
}

int rala_hip_get_pile_row_digests(rala_hip_ctx* ctx, uint64_t* fnv, uint64_t* inside, uint64_t* outside) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!ctx->initialized) return fail(ctx, RALA_HIP_EINVAL, "not initialized");
    if (!ctx->piles_resident) return fail(ctx, RALA_HIP_EINVAL, "piles live on the owning rank's context");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    return pile_row_digests(ctx, ctx->h_begin.data(), ctx->h_end.data(), ctx->h_alive.data(), fnv, inside, outside);
}

int rala_hip_get_intervals(rala_hip_ctx* ctx, int kind, uint64_t* offsets, uint32_t* pairs, uint32_t* aux) {
    if (!ctx || !offsets) return RALA_HIP_EINVAL;
    if (!ctx->initialized) return fail(ctx, RALA_HIP_EINVAL, "not initialized");
    if (kind < 0 || kind > 2) return fail(ctx, RALA_HIP_EINVAL, "bad interval kind");
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    const uint64_t n = ctx->n_reads;
    uint64_t off = 0;
    for (uint64_t r = 0; r < n; ++r) {
        offsets[r] = off;
        if (!ctx->h_alive[r]) continue;
        if (kind == 2) {
            if (!ctx->have_repeats || ctx->h_n_rep[r] == 0) continue;
            const Interval* iv = ctx->h_rep_pool.data() + ctx->h_rep_slot[r];
            const uint32_t c2 = ctx->h_n_rep[r];
            if (pairs) {
                for (uint32_t k = 0; k < c2; ++k) {
                    pairs[2 * (off + k)] = iv[k].first;
                    pairs[2 * (off + k) + 1] = iv[k].second;
                    if (aux) aux[off + k] = iv[k].aux;
                }
            }
            off += c2;
            continue;
        }
        const uint32_t cnt = kind == 0 ? ctx->h_n_pits[r] : ctx->h_n_hills[r];
        if (cnt == 0) continue;
        // hills follow the pits found by the pile kernel; the tail only ever drops pits
        // from the front segment in place, so the initial pit count is what the
        // device wrote into the pool layout: recover it from the device-side array
        const Interval* base = ctx->h_pool.data() + ctx->h_slot[r];
        const Interval* iv = base;
        if (kind == 1) iv = base + ctx->h_n_pits[r];
        if (pairs) {
            for (uint32_t k = 0; k < cnt; ++k) {
                pairs[2 * (off + k)] = iv[k].first;
                pairs[2 * (off + k) + 1] = iv[k].second;
                if (aux) aux[off + k] = iv[k].aux;
            }
        }
        off += cnt;
    }
    offsets[n] = off;
    return RALA_HIP_OK;
}

int rala_hip_get_overlaps(rala_hip_ctx* ctx, int which, uint64_t* n, uint32_t* src_index, uint32_t* a_begin,
                          uint32_t* a_end, uint32_t* b_begin, uint32_t* b_end, uint32_t* length, uint8_t* type) {
    if (!ctx || !n) return RALA_HIP_EINVAL;
    if (!ctx->constructed) return fail(ctx, RALA_HIP_EINVAL, "not constructed");
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    const std::vector<HostOvl>& v = which == 0 ? ctx->overlaps : ctx->internals;
    *n = v.size();
    if (!src_index) return RALA_HIP_OK;
    for (size_t k = 0; k < v.size(); ++k) {
        src_index[k] = v[k].src;
        if (a_begin) a_begin[k] = v[k].c.a_begin;
        if (a_end) a_end[k] = v[k].c.a_end;
        if (b_begin) b_begin[k] = v[k].c.b_begin;
        if (b_end) b_end[k] = v[k].c.b_end;
        if (length) length[k] = v[k].c.length;
        if (type) {
            // internals can outlive their piles (reference graph.cpp:849-867 never re-checks them)
            const bool live = ctx->h_alive[v[k].a] && ctx->h_alive[v[k].b];
            type[k] = live ? (uint8_t)host_type(ctx, v[k]) : (uint8_t)255;
        }
    }
    return RALA_HIP_OK;
}

int rala_hip_get_graph_size(rala_hip_ctx* ctx, uint64_t* n_nodes, uint64_t* n_edges) {
    if (!ctx || !n_nodes || !n_edges) return RALA_HIP_EINVAL;
    if (!ctx->constructed) return fail(ctx, RALA_HIP_EINVAL, "not constructed");
    if (ctx->tail_on_device) {
        *n_nodes = ctx->t_n_nodes;
        *n_edges = ctx->t_n_edges;
        return RALA_HIP_OK;
    }
    *n_nodes = ctx->node_read.size();
    *n_edges = ctx->e_src.size();
    return RALA_HIP_OK;
}

int rala_hip_get_graph(rala_hip_ctx* ctx, uint32_t* node_read, uint32_t* src, uint32_t* dst, uint32_t* len,
                       uint8_t* marks) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!ctx->constructed) return fail(ctx, RALA_HIP_EINVAL, "not constructed");
    { const int rcm = materialize_host(ctx); if (rcm != RALA_HIP_OK) return rcm; }
    if (ctx->marks_on_device) {
        HIPCHECK(hipSetDevice(ctx->device));
        ctx->e_mark.resize(ctx->t_n_edges);
        if (ctx->t_n_edges) HIPCHECK(hipMemcpy(ctx->e_mark.data(), ctx->d_tr_marks.p, ctx->t_n_edges, hipMemcpyDeviceToHost));
        marks_fetched(ctx);
    }
    if (node_read) memcpy(node_read, ctx->node_read.data(), ctx->node_read.size() * 4);
    const size_t ne = ctx->e_src.size();
    if (src) memcpy(src, ctx->e_src.data(), ne * 4);
    if (dst) memcpy(dst, ctx->e_dst.data(), ne * 4);
    if (len) memcpy(len, ctx->e_len.data(), ne * 4);
    if (marks) memcpy(marks, ctx->e_mark.data(), ne);
    return RALA_HIP_OK;
}

int rala_hip_get_timings(rala_hip_ctx* ctx, rala_hip_timings* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->tm;
    out->total_ms = ctx->tm.dedupe_ms + ctx->tm.bucket_ms + ctx->tm.pile_ms + ctx->tm.classify_ms + ctx->tm.death_ms +
                    ctx->tm.finish_ms + ctx->tm.tail_host_ms + ctx->tm.tr_ms;
    return RALA_HIP_OK;
}

int rala_hip_get_num_prefiltered(rala_hip_ctx* ctx, uint64_t* n) {
    if (!ctx || !n) return RALA_HIP_EINVAL;
    *n = ctx->n_prefiltered;
    return RALA_HIP_OK;
}

}  // extern "C"
