// What the stage files of one context's host orchestration (initialize.hip, pile_drivers.hip, construct.hip, tail_device.hip,
// tail_host.hip, sensitive.hip, transitive.hip, getters.hip) call in one another, beside the stage functions of stages.h:
// the trace, the two launch templates, the argument blocks, and the handful of functions one stage calls in another.
// Everything else of a stage file is in its anonymous namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "ctx_check.h"
#include "slots.h"
#include "stages.h"

namespace rala_hip {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// RALA_HIP_TRACE: read at every call - a process may set it late
inline bool trace_on() { return getenv("RALA_HIP_TRACE") != nullptr; }

struct Trace {
    bool on;
    double t;
    Trace() : on(trace_on()), t(now_ms()) {}
    void operator()(const char* what, size_t k = 0) {
        if (!on) return;
        const double u = now_ms();
        fprintf(stderr, "[trace] %-28s %8.3f ms  (%zu)\n", what, u - t, k);
        t = u;
    }
};

// ---- pile_drivers.hip: the position-space launch classes, the lists in global memory, rows on demand, argument blocks ------
void build_classes(rala_hip_ctx* ctx, const std::vector<uint32_t>& reads, std::vector<uint32_t>& order);
void first_big_caps(const rala_hip_ctx* ctx, uint32_t& cap_reg, uint32_t& cap_raw);
int run_position_kernel(rala_hip_ctx* ctx, const PileArgs& a, const std::vector<uint32_t>& reads);
int run_unbounded_piles(rala_hip_ctx* ctx, PileArgs a, uint32_t count, uint32_t* count_dev);

// where the primary bound events are: in fixed slots (cnt: events per read) or behind the CSR d_ev_off (cnt null), which
// counts in units of 1 << shift events.  rala_hip_initialize passes what it has just decided, later callers the context's.
struct PrimaryEvents {
    const uint32_t* ev;
    const uint32_t* cnt;
    uint32_t shift;
};
PrimaryEvents primary_events(rala_hip_ctx* ctx, bool fixed, uint32_t shift);
PileArgs pile_args(rala_hip_ctx* ctx, const PrimaryEvents& pe);
RepeatArgs repeat_args(rala_hip_ctx* cl);
uint32_t grown_pool_size(uint32_t used, uint32_t cap);

// rows start on 128-byte boundaries in the scratch, as they do in the resident buffer
inline uint64_t scratch_row_elems(uint32_t len) { return ((uint64_t)len + 63u) & ~(uint64_t)63u; }
uint64_t rows_scratch_cap(const rala_hip_ctx* ctx);
int materialize_rows(rala_hip_ctx* ctx, const uint32_t* reads, uint32_t first, uint32_t count, bool with_sens, hipStream_t st);

// A position-space kernel (PileArgs or RepeatArgs) over `reads`, grouped by LDS image size, on stream st: one launch(a, grid,
// in_lds) per class, a's order / n_items / lw / slab set.  big: with the region / interval lists in global memory at a's
// sizes, words(..) words per workgroup (a.big_space is set here).  Nothing here waits for another stream; st is waited for.
// who: the caller's name in the trace (null: no lines).
template <class Args, class Launch>
int launch_by_class(rala_hip_ctx* ctx, Args a, const std::vector<uint32_t>& reads, bool big, uint64_t (*words)(uint32_t, uint32_t, uint32_t),
                    hipStream_t st, const char* who, Launch launch) {
    if (reads.empty()) return RALA_HIP_OK;
    Trace trc;
    std::vector<uint32_t> order;
    build_classes(ctx, reads, order);
    if (who) trc((std::string(who) + ": classes").c_str(), reads.size());
    HIPCHECK(ctx->d_order.ensure(order.size() + 1));
    HIPCHECK(hipMemcpyAsync(ctx->d_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    const uint64_t big_words = big ? words(a.big_cap_reg, a.big_cap_list, a.big_cap_raw) : 0;
    for (const LaunchClass& c : ctx->classes) {
        uint32_t grid = c.count;
        if (!c.in_lds) grid = std::min<uint32_t>(c.count, 512);
        if (big) {
            grid = std::min<uint32_t>(grid, 64);
            HIPCHECK(ctx->d_big_space.ensure((size_t)(big_words * grid)));
            a.big_space = ctx->d_big_space.p;
        }
        if (!c.in_lds) HIPCHECK(ctx->d_slab.ensure((size_t)grid * 3 * c.lw));
        a.order = ctx->d_order.p + c.first;
        a.n_items = c.count;
        a.lw = c.lw;
        a.slab = ctx->d_slab.p;
        launch(a, grid, c.in_lds);
    }
    // `order` is pageable host memory.  Not stream_sync: st may be a side stream, and this wait delivers no copy that
    // d2h_small staged - none is pending at a caller today, and one queued in front of a call would wait for the next stream_sync
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipGetLastError());
    if (who) trc((std::string(who) + ": kernels").c_str(), ctx->classes.size());
    return RALA_HIP_OK;
}

// The reads a position-space kernel noted in d_big_list[0] (`count` of them): once more, with the region lists and raw
// intervals in global memory; lists that still do not fit are doubled for the reads concerned until they do (the reference
// keeps them in vectors, pile.cpp:66, 359, 448).  run(reads, note_in, cap_reg, cap_list, cap_raw) runs them on stream st and
// waits for it; the reads that still do not fit are noted in note_in, *count_dev of them, with their bits in *status_dev
// (which keeps its pool-capacity bit).  The first cap_list is list_factor * cap_reg.  Copies and clears are on st: the
// caller's other streams go on beside.  what: the caller's word in the trace; left_text: its error text.
template <class Run>
int run_until_lists_fit(rala_hip_ctx* ctx, uint32_t count, uint32_t* count_dev, uint32_t* status_dev, uint32_t list_factor, hipStream_t st,
                        const char* what, const char* left_text, Run run) {
    uint32_t cap_reg, cap_raw;
    first_big_caps(ctx, cap_reg, cap_raw);
    uint32_t cap_list = list_factor * cap_reg;
    int from = 0;
    while (count) {
        std::vector<uint32_t> reads(count);
        HIPCHECK(hipMemcpyAsync(reads.data(), ctx->d_big_list[from].p, (size_t)count * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        std::sort(reads.begin(), reads.end());
        HIPCHECK(ctx->d_big_list[from ^ 1].ensure(ctx->n_reads + 1));
        // (the lists' bits of the status word start every round at zero; other kernels may be setting the pool's bit meanwhile)
        launch_status_clear(status_dev, kErrRegionCapacity | kErrRawCapacity, count_dev, st);
        const int rc = run(reads, ctx->d_big_list[from ^ 1].p, cap_reg, cap_list, cap_raw);
        if (rc != RALA_HIP_OK) return rc;
        uint32_t left = 0, status = 0;
        HIPCHECK(hipMemcpyAsync(&left, count_dev, 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(&status, status_dev, 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        HIPCHECK(hipGetLastError());
        if (trace_on()) {
            fprintf(stderr, "[trace] %slists in global memory: %u reads at %u regions / %u raw intervals, %u left (status %u)\n", what, count,
                    cap_reg, cap_raw, left, status);
        }
        if (left && !(status & (kErrRegionCapacity | kErrRawCapacity))) return fail(ctx, RALA_HIP_EDEVICE, left_text);
        if (status & kErrRegionCapacity) {
            if (cap_reg > (1u << 26)) return fail(ctx, RALA_HIP_ENOMEM, "slope-region lists beyond 2^26 entries");
            cap_reg *= 2; cap_list *= 2;
        }
        if (status & kErrRawCapacity) {
            if (cap_raw > (1u << 28)) return fail(ctx, RALA_HIP_ENOMEM, "interval lists beyond 2^28 entries");
            cap_raw *= 2;
        }
        count = left;
        from ^= 1;
    }
    // (the lists' bits are no error of the call any more)
    launch_status_clear(status_dev, kErrRegionCapacity | kErrRawCapacity, nullptr, st);
    HIPCHECK(hipStreamSynchronize(st));
    return RALA_HIP_OK;
}

// ---- tail_device.hip: the survivor lists on the device, the chimera stage and the graph behind it ---------------------------
Survivors survivors_of(uint32_t* const c32[8], uint8_t* strand, uint8_t* type);
Survivors survivors_view(rala_hip_ctx* ctx);
HostOvl host_item(const Survivors& sv, size_t k);
TailList tail_list(rala_hip_ctx* ctx);
int scan_space(rala_hip_ctx* ctx, uint32_t scans, uint64_t items, ScanSpace& sp, FillList* fills = nullptr);
int tail_components(rala_hip_ctx* ctx, const TailList& L, uint32_t n_alive, bool touched_cleared = false);
int gpu_tail_part_a(rala_hip_ctx* ctx);
int gpu_tail_part_b(rala_hip_ctx* ctx);
int gpu_tail_run(rala_hip_ctx* ctx);
int materialize_host(rala_hip_ctx* ctx);

// ---- tail_host.hip: the same stage on the host (use_gpu_tail = 0) ------------------------------------------------------------
uint32_t host_type(rala_hip_ctx* ctx, const HostOvl& o);
int component_medians(rala_hip_ctx* ctx, std::vector<uint32_t>& members, std::vector<uint16_t>& med_of_member);
int preprocess_chimeras(rala_hip_ctx* ctx);
void build_graph(rala_hip_ctx* ctx);

// ---- sensitive.hip -----------------------------------------------------------------------------------------------------------
int download_repeat_hills(rala_hip_ctx* ctx);
int preprocess_repeats(rala_hip_ctx* cs, rala_hip_ctx* cl, Comm* comm, const rala_hip_overlaps* sens, uint64_t n_sens,
                       bool device_lists);

}  // namespace rala_hip
