// librala_hip: the drivers of the position-space kernels that more than one stage uses (orchestration.h) - launch classes, the
// noted reads with their lists in global memory, rows on demand (option pile_rows = 0), the kernels' argument blocks - and, of
// stages.h, pile_row_digests and pile_row_to_host.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orchestration.h"

using namespace rala_hip;

// ---- launch classes of the position-space kernel: reads grouped by LDS image size ------
void rala_hip::build_classes(rala_hip_ctx* ctx, const std::vector<uint32_t>& reads, std::vector<uint32_t>& order) {
    static const uint32_t kLw[] = {8192, 10240, 12288, 14336, 16384, 20480, 24576};
    const int n_lds = (int)(sizeof(kLw) / sizeof(kLw[0]));
    std::vector<std::vector<uint32_t>> bins(n_lds + 1);
    uint32_t max_long = 0;
    // a handful of reads (what the run-space chain hands on: a dozen at C3): ONE launch at the size of the longest - three
    // launches of four workgroups each are three times the latency of one
    int only = -1;
    if (reads.size() <= 32) {
        uint32_t top = 0;
        for (uint32_t r : reads) top = std::max(top, ctx->h_read_len[r]);
        only = n_lds;
        if ((int64_t)top <= ctx->max_lds_read_len) {
            for (int c = 0; c < n_lds; ++c) {
                if (pile_lw_for(top) <= kLw[c]) { only = c; break; }
            }
        }
    }
    for (uint32_t r : reads) {
        const uint32_t len = ctx->h_read_len[r];
        const uint32_t lw = pile_lw_for(len);
        int k = n_lds;
        if ((int64_t)len <= ctx->max_lds_read_len) {
            for (int c = 0; c < n_lds; ++c) {
                if (lw <= kLw[c]) { k = c; break; }
            }
        }
        if (only >= 0) k = only;
        bins[k].push_back(r);
        if (k == n_lds) max_long = std::max(max_long, lw);
    }
    ctx->classes.clear();
    order.clear();
    // big classes first: their workgroups are the long poles
    for (int k = n_lds; k >= 0; --k) {
        if (bins[k].empty()) continue;
        LaunchClass c;
        c.in_lds = k < n_lds;
        c.lw = c.in_lds ? kLw[k] : max_long;
        c.first = (uint32_t)order.size();
        c.count = (uint32_t)bins[k].size();
        // longest first (only a scheduling matter): counting sort on length / 64
        {
            const std::vector<uint32_t>& v = bins[k];
            uint32_t top = 0;
            for (uint32_t r : v) top = std::max(top, ctx->h_read_len[r] >> 6);
            std::vector<uint32_t> at(top + 2, 0);
            for (uint32_t r : v) ++at[top - (ctx->h_read_len[r] >> 6) + 1];
            for (uint32_t b = 0; b <= top; ++b) at[b + 1] += at[b];
            const size_t base = order.size();
            order.resize(base + v.size());
            for (uint32_t r : v) order[base + at[top - (ctx->h_read_len[r] >> 6)]++] = r;
        }
        ctx->classes.push_back(c);
    }
}

// the pile kernel in position space over `reads` (all of them, or the run kernel's overflow), on the main stream
// a.big_cap_reg != 0: with the region / interval lists in global memory at those sizes
int rala_hip::run_position_kernel(rala_hip_ctx* ctx, const PileArgs& a, const std::vector<uint32_t>& reads) {
    hipStream_t s = ctx->stream;
    return launch_by_class(ctx, a, reads, a.big_cap_reg != 0, pile_big_words, s, nullptr, [&](const PileArgs& c, uint32_t grid, bool in_lds) {
        launch_pile_build_annotate(c, grid, in_lds, s);
        ++ctx->tm.pile_launches;
    });
}

// first sizes of the lists in global memory (the position-space kernels' LDS lists hold 192 regions per flag list and 64 raw
// intervals); the option debug_big_caps = regions << 32 | raw intervals makes tests start lower
void rala_hip::first_big_caps(const rala_hip_ctx* ctx, uint32_t& cap_reg, uint32_t& cap_raw) {
    cap_reg = 1024; cap_raw = 4096;
    if (ctx->debug_big_caps) {
        cap_reg = std::max<uint32_t>(4, (uint32_t)((uint64_t)ctx->debug_big_caps >> 32));
        cap_raw = std::max<uint32_t>(4, (uint32_t)((uint64_t)ctx->debug_big_caps & 0xFFFFFFFFu));
    }
}

// the pile kernel's noted reads (initialize; a: the call's arguments), on the main stream
int rala_hip::run_unbounded_piles(rala_hip_ctx* ctx, PileArgs a, uint32_t count, uint32_t* count_dev) {
    ctx->tm.pile_unbounded_reads += count;
    a.big_count = count_dev;
    a.n_items_dev = nullptr;
    return run_until_lists_fit(ctx, count, count_dev, a.error, 4, ctx->stream, "", "position-space kernel: reads left without a reason",
                               [&](const std::vector<uint32_t>& reads, uint32_t* note_in, uint32_t cap_reg, uint32_t cap_list, uint32_t cap_raw) {
                                   a.big_list = note_in;
                                   a.big_cap_reg = cap_reg; a.big_cap_list = cap_list; a.big_cap_raw = cap_raw;
                                   return run_position_kernel(ctx, a, reads);
                               });
}

// ---- argument blocks ------------------------------------------------------------------------------------------------------
PrimaryEvents rala_hip::primary_events(rala_hip_ctx* ctx, bool fixed, uint32_t shift) {
    return {fixed ? ctx->d_ev_fixed.p : ctx->d_ev.p, fixed ? ctx->d_cursor.p : nullptr, shift};
}

// what the pile kernels of initialize and of the sensitive pass share: the reads, their rows (none with pile_rows = 0), the
// primary events, the per-read results; everything else zero
PileArgs rala_hip::pile_args(rala_hip_ctx* ctx, const PrimaryEvents& pe) {
    PileArgs a{};
    a.read_len = ctx->d_read_len.p; a.pile_off = ctx->d_pile_off.p; a.pile = ctx->rowless ? nullptr : ctx->d_pile.p;
    a.ev_off = ctx->d_ev_off.p; a.ev = pe.ev; a.ev_cnt = pe.cnt; a.ev_stride = kRunEventCapBig; a.ev_shift = pe.shift;
    a.begin = ctx->d_begin.p; a.end = ctx->d_end.p; a.median = ctx->d_median.p; a.p10 = ctx->d_p10.p;
    return a;
}

// the repeat-hill kernel's arguments on the context that holds the piles (ev_off / ev: the caller's)
RepeatArgs rala_hip::repeat_args(rala_hip_ctx* cl) {
    RepeatArgs a{};
    a.read_len = cl->d_read_len.p; a.pile_off = cl->d_pile_off.p; a.pile = cl->d_pile.p;
    a.begin = cl->d_begin.p; a.end = cl->d_end.p; a.median = cl->d_median.p; a.p10 = cl->d_p10.p;
    a.dataset_median = cl->d_dataset_median.p; a.n_rep = cl->d_n_rep.p; a.rep_slot = cl->d_rep_slot.p;
    a.pool = cl->d_rep_pool.p; a.pool_count = cl->d_small.p + kSensPoolCount; a.pool_cap = cl->rep_pool_cap;
    a.error = cl->d_small.p + kSensStatus;
    return a;
}

// the pool a stage needs when its kernels counted `used` entries into one of `cap`: that and an eighth more (the slots of
// reads that ran twice are not handed back); 0: no size helps (the counter did not pass the capacity, or 2^32 entries)
uint32_t rala_hip::grown_pool_size(uint32_t used, uint32_t cap) {
    const uint64_t need = (uint64_t)used + used / 8 + 1024;
    return used <= cap || need > 0xFFFFFFF0ull ? 0u : (uint32_t)need;
}

// ---- rows on demand (option pile_rows = 0; pile_rows_kernel.hip) -------------------------------------------------------
// what a batch of rebuilt rows may take, in values: the option, or the longest row where that is larger
uint64_t rala_hip::rows_scratch_cap(const rala_hip_ctx* ctx) {
    return std::max<uint64_t>(((uint64_t)ctx->pile_rows_scratch_mb << 20) / sizeof(uint16_t), scratch_row_elems(ctx->max_read_len));
}
// The rows of `count` reads - reads[0 .. count) (host), or first, first + 1, ... where reads is null - rebuilt into
// ctx->d_rows_scratch on stream st; ctx->d_rows_off[read] says where (what pile_off is to the resident rows).  with_sens: the
// sensitive bounds of the last sensitive construct on top (Pile::add_layers a second time, graph.cpp:941-969).  The stream is
// waited for.
int rala_hip::materialize_rows(rala_hip_ctx* ctx, const uint32_t* reads, uint32_t first, uint32_t count, bool with_sens, hipStream_t st) {
    if (count == 0) return RALA_HIP_OK;
    if (!ctx->ev_ready) return fail(ctx, RALA_HIP_EINVAL, "the bound events of rala_hip_initialize are gone: no row can be rebuilt");
    const uint64_t n = ctx->n_reads;
    HIPCHECK(ctx->d_rows_off.ensure(n + 1));
    ctx->h_rows_off.resize(n);
    uint64_t total = 0;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t r = reads ? reads[i] : first + i;
        if (r >= n) return fail(ctx, RALA_HIP_EINVAL, "bad read in a list of rows");
        ctx->h_rows_off[r] = total;
        total += scratch_row_elems(ctx->h_read_len[r]);
        lo = std::min(lo, r); hi = std::max(hi, r);
    }
    HIPCHECK(ctx->d_rows_scratch.ensure(total + 64));
    HIPCHECK(hipMemcpyAsync(ctx->d_rows_off.p + lo, ctx->h_rows_off.data() + lo, (size_t)(hi - lo + 1) * 8, hipMemcpyHostToDevice, st));
    if (reads) {
        HIPCHECK(ctx->d_rows_list.ensure(count));
        HIPCHECK(hipMemcpyAsync(ctx->d_rows_list.p, reads, (size_t)count * 4, hipMemcpyHostToDevice, st));
    }
    RowsArgs ra;
    ra.reads = reads ? ctx->d_rows_list.p : nullptr; ra.first = first; ra.n_items = count;
    ra.read_len = ctx->d_read_len.p; ra.dst_off = ctx->d_rows_off.p; ra.rows = ctx->d_rows_scratch.p;
    const PrimaryEvents pe = primary_events(ctx, ctx->ev_fixed, ctx->ev_shift);
    ra.ev_off = ctx->d_ev_off.p; ra.ev = pe.ev; ra.ev_cnt = pe.cnt; ra.ev_stride = kRunEventCapBig; ra.ev_shift = pe.shift;
    ra.sens_off = with_sens ? ctx->d_sens_off.p : nullptr; ra.sens_ev = with_sens ? ctx->d_sens_ev.p : nullptr;
    launch_pile_rows(ra, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));             // (`reads` is pageable host memory)
    ctx->rows_materialised += count;
    return RALA_HIP_OK;
}

// every row of cl where it lies, under the regions that apply (the getters' view: rala_hip_get_pile_data zeroes outside them)
int rala_hip::pile_row_digests(rala_hip_ctx* ctx, const uint32_t* begin, const uint32_t* end, const uint8_t* alive, uint64_t* fnv,
                               uint64_t* inside, uint64_t* outside) {
    const uint64_t n = ctx->n_reads;
    if (n == 0) return RALA_HIP_OK;
    HIPCHECK(hipSetDevice(ctx->device));
    DevBuf<uint32_t> d_be;
    DevBuf<uint8_t> d_al;
    DevBuf<uint64_t> d_out;
    HIPCHECK(d_be.ensure(2 * n)); HIPCHECK(d_al.ensure(n)); HIPCHECK(d_out.ensure(3 * n));
    HIPCHECK(hipMemcpy(d_be.p, begin, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_be.p + n, end, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_al.p, alive, n, hipMemcpyHostToDevice));
    hipStream_t s = ctx->stream;
    if (ctx->rowless) {
        // no row is resident: the reads in batches of what the scratch holds, every batch rebuilt and hashed where it lies.
        // Nothing is stored, so nothing is stored outside a region: `outside` is 0 by definition.
        const uint64_t cap = rows_scratch_cap(ctx);
        for (uint64_t r0 = 0; r0 < n;) {
            uint64_t r1 = r0, total = 0;
            do total += scratch_row_elems(ctx->h_read_len[r1++]);
            while (r1 < n && total + scratch_row_elems(ctx->h_read_len[r1]) <= cap);
            const int rc = materialize_rows(ctx, nullptr, (uint32_t)r0, (uint32_t)(r1 - r0), ctx->sens_csr_ready, s);
            if (rc != RALA_HIP_OK) return rc;
            launch_pile_row_digests(ctx->d_rows_scratch.p, ctx->d_rows_off.p + r0, ctx->d_read_len.p + r0, d_be.p + r0, d_be.p + n + r0, d_al.p + r0,
                                    (uint32_t)(r1 - r0), fnv ? d_out.p + r0 : nullptr, inside ? d_out.p + n + r0 : nullptr, nullptr, s);
            HIPCHECK(hipGetLastError());
            HIPCHECK(stream_sync(ctx, s));          // (the next batch overwrites the scratch)
            r0 = r1;
        }
        if (outside) std::fill(outside, outside + n, (uint64_t)0);
    } else {
    launch_pile_row_digests(ctx->d_pile.p, ctx->d_pile_off.p, ctx->d_read_len.p, d_be.p, d_be.p + n, d_al.p, (uint32_t)n,
                            fnv ? d_out.p : nullptr, inside ? d_out.p + n : nullptr, outside ? d_out.p + 2 * n : nullptr, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(stream_sync(ctx, s));
    }
    if (fnv) HIPCHECK(hipMemcpy(fnv, d_out.p, n * 8, hipMemcpyDeviceToHost));
    if (inside) HIPCHECK(hipMemcpy(inside, d_out.p + n, n * 8, hipMemcpyDeviceToHost));
    if (outside && !ctx->rowless) HIPCHECK(hipMemcpy(outside, d_out.p + 2 * n, n * 8, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

int rala_hip::pile_row_to_host(rala_hip_ctx* ctx, uint64_t read, uint16_t* data) {
    const uint32_t n = ctx->h_read_len[read];
    if (!ctx->rowless) {
        HIPCHECK(ctx->d_pile.copy_to_host(data, ctx->h_pile_off[read], n));
        return RALA_HIP_OK;
    }
    const int rc = materialize_rows(ctx, nullptr, (uint32_t)read, 1, ctx->sens_csr_ready, ctx->stream);
    if (rc != RALA_HIP_OK) return rc;
    if (n) HIPCHECK(hipMemcpy(data, ctx->d_rows_scratch.p, (size_t)n * 2, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}
