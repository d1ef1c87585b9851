// rala_hip_layout_batch: the force-directed layout of all components of a round in one call (reference rvaser/rala
// src/graph.cpp:1132-1226, once per component of the loop at :1106).  rala_hip_layout (at the end of this file) costs four copies, one
// launch per step, two copies and a wait PER COMPONENT; a graph with repeats, low-coverage breaks and plasmids has hundreds
// of small components per round and five rounds.  Here: one packed upload, one launch per size class for the components a
// workgroup can hold (layout_fused_kernel), one launch per step for all larger ones together (layout_batch_step_kernel),
// one download, one wait.  The arithmetic per point is that of layout_step_kernel, so the results are the same bits.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "ctx_check.h"
#include "stages.h"

using namespace rala_hip;

namespace {

size_t align8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

}  // namespace

int rala_hip_layout_batch(rala_hip_ctx* ctx, uint32_t n_components, const uint32_t* comp_off, double* x, double* y,
                          const uint32_t* adj_off, const uint32_t* adj, const double* k, uint32_t iterations, double t,
                          double dt) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (n_components && !comp_off) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: comp_off is null");
    // ---- everything is checked before anything is enqueued ----
    const uint32_t C = n_components;
    if (C && comp_off[0] != 0) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: comp_off does not start at 0");
    for (uint32_t c = 0; c < C; ++c) {
        if (comp_off[c + 1] < comp_off[c]) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: comp_off decreases");
    }
    const size_t N = C ? comp_off[C] : 0;
    if (N && (!x || !y || !adj_off || !k)) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: a null array");
    if (N && adj_off[0] != 0) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: adj_off does not start at 0");
    for (size_t p = 0; p < N; ++p) {
        if (adj_off[p + 1] < adj_off[p]) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: adj_off decreases");
    }
    const size_t A = N ? adj_off[N] : 0;
    if (A && !adj) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: adj is null");
    for (uint32_t c = 0; c < C && N; ++c) {
        const uint32_t n_c = comp_off[c + 1] - comp_off[c];
        for (size_t a = adj_off[comp_off[c]]; a < adj_off[comp_off[c + 1]]; ++a) {
            if (adj[a] > n_c) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: a partner index beyond its component");
        }
    }

    // ---- which component takes which path ----
    const uint32_t fused_max = (uint32_t)ctx->layout_fused_max;
    std::vector<uint32_t> list256, list1024, tiles;
    rala_hip_layout_info info = {};
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t n_c = comp_off[c + 1] - comp_off[c];
        if (n_c == 0) {
            ++info.components_empty;
        } else if (n_c <= fused_max && n_c <= 256) {
            list256.push_back(c);
            info.points_fused_256 += n_c;
        } else if (n_c <= fused_max) {
            list1024.push_back(c);
            info.points_fused_1024 += n_c;
        } else {
            for (uint32_t first = 0; first < n_c; first += kLayoutTile) { tiles.push_back(c); tiles.push_back(first); }
            ++info.components_stepped;
            info.points_stepped += n_c;
        }
    }
    info.components_fused_256 = (uint32_t)list256.size();
    info.components_fused_1024 = (uint32_t)list1024.size();
    const size_t T = tiles.size() / 2;
    if (T > 0x7FFFFFFFull) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_layout_batch: too many points for one launch");
    info.step_tiles = (uint32_t)T;
    if (N == 0 || iterations == 0) {
        ctx->layout_info = info;
        return RALA_HIP_OK;
    }
    info.launches = (list256.empty() ? 0u : 1u) + (list1024.empty() ? 0u : 1u) + (T ? iterations : 0u);

    // ---- one block: [x | y | k] doubles, [comp_off | adj_off | adj | list256 | list1024 | pad | tiles] words: the upload;
    //      behind it the second position buffers ----
    const size_t o_x = 0, o_y = o_x + N * 8, o_k = o_y + N * 8, o_comp = o_k + (size_t)C * 8;
    const size_t o_adj_off = o_comp + ((size_t)C + 1) * 4, o_adj = o_adj_off + (N + 1) * 4, o_l256 = o_adj + A * 4;
    const size_t o_l1024 = o_l256 + list256.size() * 4, o_tiles = align8(o_l1024 + list1024.size() * 4);
    const size_t upload = o_tiles + T * 8, o_x2 = align8(upload), o_y2 = o_x2 + N * 8, total = o_y2 + N * 8;
    HIPCHECK(hipSetDevice(ctx->device));
    for (auto& e : ctx->ev_layout) if (!e) HIPCHECK(hipEventCreate(&e));
    HIPCHECK(ctx->d_layout_batch.ensure(total));
    HIPCHECK(ctx->p_layout_batch.ensure(upload));
    unsigned char* const h = ctx->p_layout_batch.p;
    unsigned char* const d = ctx->d_layout_batch.p;
    memcpy(h + o_x, x, N * 8);
    memcpy(h + o_y, y, N * 8);
    memcpy(h + o_k, k, (size_t)C * 8);
    memcpy(h + o_comp, comp_off, ((size_t)C + 1) * 4);
    memcpy(h + o_adj_off, adj_off, (N + 1) * 4);
    if (A) memcpy(h + o_adj, adj, A * 4);
    if (!list256.empty()) memcpy(h + o_l256, list256.data(), list256.size() * 4);
    if (!list1024.empty()) memcpy(h + o_l1024, list1024.data(), list1024.size() * 4);
    if (T) memcpy(h + o_tiles, tiles.data(), T * 8);

    hipStream_t s = ctx->stream;
    HIPCHECK(hipMemcpyAsync(d, h, upload, hipMemcpyHostToDevice, s));
    double* const px[2] = {(double*)(d + o_x), (double*)(d + o_x2)};
    double* const py[2] = {(double*)(d + o_y), (double*)(d + o_y2)};
    const double* const d_k = (const double*)(d + o_k);
    const uint32_t* const d_comp = (const uint32_t*)(d + o_comp);
    const uint32_t* const d_adj_off = (const uint32_t*)(d + o_adj_off);
    const uint32_t* const d_adj = (const uint32_t*)(d + o_adj);
    // where the stepped components end up after `iterations` swaps; the fused ones write there directly
    const int last = (int)(iterations & 1u);
    HIPCHECK(hipEventRecord(ctx->ev_layout[0], s));
    launch_layout_fused(256, (uint32_t)list256.size(), (const uint32_t*)(d + o_l256), d_comp, px[0], py[0], px[last], py[last],
                        d_adj_off, d_adj, d_k, iterations, t, dt, s);
    launch_layout_fused(1024, (uint32_t)list1024.size(), (const uint32_t*)(d + o_l1024), d_comp, px[0], py[0], px[last],
                        py[last], d_adj_off, d_adj, d_k, iterations, t, dt, s);
    if (T) {
        int cur = 0;
        double t_step = t;
        for (uint32_t it = 0; it < iterations; ++it) {
            launch_layout_batch_step((uint32_t)T, (const uint2*)(d + o_tiles), d_comp, px[cur], py[cur], px[cur ^ 1], py[cur ^ 1],
                                     d_adj_off, d_adj, d_k, t_step, s);
            cur ^= 1;
            t_step -= dt;
        }
    }
    HIPCHECK(hipEventRecord(ctx->ev_layout[1], s));
    // x and y of a buffer lie side by side: one copy (into the pinned block, which the upload has left by now)
    HIPCHECK(hipMemcpyAsync(h, px[last], 2 * N * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    memcpy(x, h, N * 8);
    memcpy(y, h + N * 8, N * 8);
    HIPCHECK(hipEventElapsedTime(&info.device_ms, ctx->ev_layout[0], ctx->ev_layout[1]));
    ctx->layout_info = info;
    return RALA_HIP_OK;
}

int rala_hip_get_layout_info(rala_hip_ctx* ctx, rala_hip_layout_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->layout_info;
    return RALA_HIP_OK;
}

int rala_hip_layout(rala_hip_ctx* ctx, uint32_t n, double* x, double* y, const uint32_t* adj_off, const uint32_t* adj,
                    uint32_t iterations, double k, double t, double dt) {
    if (!ctx || (n && (!x || !y || !adj_off))) return RALA_HIP_EINVAL;
    if (n == 0) return RALA_HIP_OK;
    const uint32_t n_adj = adj_off[n];
    if (n_adj && !adj) return RALA_HIP_EINVAL;
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (int b = 0; b < 4; ++b) HIPCHECK(ctx->d_layout[b].ensure(n));
    HIPCHECK(ctx->d_layout_adj[0].ensure(n + 1)); HIPCHECK(ctx->d_layout_adj[1].ensure(n_adj + 1));
    HIPCHECK(hipMemcpyAsync(ctx->d_layout[0].p, x, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_layout[1].p, y, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_layout_adj[0].p, adj_off, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_adj) HIPCHECK(hipMemcpyAsync(ctx->d_layout_adj[1].p, adj, (size_t)n_adj * 4, hipMemcpyHostToDevice, s));
    int cur = 0;
    for (uint32_t it = 0; it < iterations; ++it) {
        launch_layout_step(n, ctx->d_layout[2 * cur].p, ctx->d_layout[2 * cur + 1].p, ctx->d_layout[2 * (cur ^ 1)].p,
                           ctx->d_layout[2 * (cur ^ 1) + 1].p, ctx->d_layout_adj[0].p, ctx->d_layout_adj[1].p, k, t, s);
        cur ^= 1;
        t -= dt;
    }
    HIPCHECK(hipMemcpyAsync(x, ctx->d_layout[2 * cur].p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(y, ctx->d_layout[2 * cur + 1].p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    return RALA_HIP_OK;
}
