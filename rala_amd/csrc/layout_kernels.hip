// Force-directed layout step of Graph::postprocess (reference rvaser/rala
// src/graph.cpp:1132-1226): every point is pushed away from every other point of its component
// by k^2 / d^2 and pulled towards its neighbours (graph edges and removed transitive edges) by
// d / k, then moved by t along the normalised sum.  FP64 throughout, in the reference's order
// of operations and with one accumulator per point walked in ascending point order, so the
// result is bit-identical to a sequential evaluation (no FMA contraction: the library is built
// with -ffp-contract=off; sqrt and division are correctly rounded).
//
// O(n^2) per step: one thread per point, the other points streamed through LDS in tiles.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rala_hip {

namespace {

constexpr int kTile = 256;
static_assert(kTile == (int)kLayoutTile, "the tile table of rala_hip_layout_batch is built for this tile");

__global__ __launch_bounds__(kTile) void layout_step_kernel(uint32_t n, const double* __restrict__ x,
                                                            const double* __restrict__ y, double* __restrict__ x_out,
                                                            double* __restrict__ y_out,
                                                            const uint32_t* __restrict__ adj_off,
                                                            const uint32_t* __restrict__ adj, double k, double t) {
    __shared__ double sx[kTile], sy[kTile];
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const double px = i < n ? x[i] : 0.0, py = i < n ? y[i] : 0.0;
    double ax = 0.0, ay = 0.0;
    for (uint32_t m0 = 0; m0 < n; m0 += kTile) {
        const uint32_t m = m0 + threadIdx.x;
        sx[threadIdx.x] = m < n ? x[m] : 0.0;
        sy[threadIdx.x] = m < n ? y[m] : 0.0;
        __syncthreads();
        const uint32_t cnt = n - m0 < (uint32_t)kTile ? n - m0 : (uint32_t)kTile;
        if (i < n) {
            for (uint32_t j = 0; j < cnt; ++j) {
                if (m0 + j == i) continue;
                const double dx = px - sx[j], dy = py - sy[j];
                double distance = sqrt(dx * dx + dy * dy);
                if (distance < 0.01) distance = 0.01;
                const double s = (k * k) / (distance * distance);
                ax = ax + dx * s;
                ay = ay + dy * s;
            }
        }
        __syncthreads();
    }
    if (i >= n) return;
    for (uint32_t a = adj_off[i]; a < adj_off[i + 1]; ++a) {
        const uint32_t m = adj[a];
        const double mx = m < n ? x[m] : 0.0, my = m < n ? y[m] : 0.0;     // index n: the origin
        const double dx = px - mx, dy = py - my;
        double distance = sqrt(dx * dx + dy * dy);
        if (distance < 0.01) distance = 0.01;
        const double s = -1. * distance / k;
        ax = ax + dx * s;
        ay = ay + dy * s;
    }
    double length = sqrt(ax * ax + ay * ay);
    if (length < 0.01) length = 0.1;                    // sic (graph.cpp:1208-1210)
    const double s = t / length;
    x_out[i] = px + ax * s;
    y_out[i] = py + ay * s;
}

// ---- many components in one call (rala_hip_layout_batch) ------------------------------------------
// Real graphs give hundreds of small tangles per round; one launch chain per tangle is launch and
// sync latency only.  Two kernels, both with the arithmetic of layout_step_kernel above, operation
// for operation (one ax / ay pair per point, repulsion over ascending j with j == i skipped, then
// the attraction list in order, the same clamps), so a component's result does not depend on the
// path it took.

// (a) A component of at most BLOCK points: one workgroup, every step inside the launch.  The
// positions live in LDS, double-buffered (x and y of a point side by side: one 16-byte read per
// partner); one barrier per step - a step reads buffer `cur` only and writes buffer `cur ^ 1` only,
// and nobody passes the barrier before everybody has finished reading.  The step length is t,
// t - dt, (t - dt) - dt, ... as the host loop of rala_hip_layout forms it.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void layout_fused_kernel(const uint32_t* __restrict__ list,
                                                             const uint32_t* __restrict__ comp_off,
                                                             const double* x, const double* y, double* x_out,
                                                             double* y_out,        // (may be x, y: a point is its thread's)
                                                             const uint32_t* __restrict__ adj_off,
                                                             const uint32_t* __restrict__ adj,
                                                             const double* __restrict__ k_of, uint32_t iterations,
                                                             double t, double dt) {
    __shared__ double2 pos[2][BLOCK];
    const uint32_t c = list[blockIdx.x];
    const uint32_t base = comp_off[c], n = comp_off[c + 1] - base;      // n <= BLOCK (the host sorted it here)
    const uint32_t i = threadIdx.x;
    const bool mine = i < n;
    const double k = k_of[c];
    uint32_t a0 = 0, a1 = 0;
    double px = 0.0, py = 0.0;
    if (mine) {
        px = x[base + i]; py = y[base + i];
        a0 = adj_off[base + i]; a1 = adj_off[base + i + 1];
        pos[0][i] = make_double2(px, py);
    }
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t it = 0; it < iterations; ++it) {
        if (mine) {
            const double2* __restrict__ p = pos[cur];
            double ax = 0.0, ay = 0.0;
            for (uint32_t j = 0; j < n; ++j) {
                if (j == i) continue;
                const double2 q = p[j];
                const double dx = px - q.x, dy = py - q.y;
                double distance = sqrt(dx * dx + dy * dy);
                if (distance < 0.01) distance = 0.01;
                const double s = (k * k) / (distance * distance);
                ax = ax + dx * s;
                ay = ay + dy * s;
            }
            for (uint32_t a = a0; a < a1; ++a) {
                const uint32_t m = adj[a];
                double mx = 0.0, my = 0.0;                              // index n: the origin
                if (m < n) { const double2 q = p[m]; mx = q.x; my = q.y; }
                const double dx = px - mx, dy = py - my;
                double distance = sqrt(dx * dx + dy * dy);
                if (distance < 0.01) distance = 0.01;
                const double s = -1. * distance / k;
                ax = ax + dx * s;
                ay = ay + dy * s;
            }
            double length = sqrt(ax * ax + ay * ay);
            if (length < 0.01) length = 0.1;                            // sic (graph.cpp:1208-1210)
            const double s = t / length;
            px = px + ax * s;
            py = py + ay * s;
            pos[cur ^ 1][i] = make_double2(px, py);
        }
        __syncthreads();
        cur ^= 1;
        t -= dt;
    }
    if (mine) { x_out[base + i] = px; y_out[base + i] = py; }
}

// (b) One step of every larger component: a workgroup per tile {component, first local point},
// which streams its own component's points through LDS exactly as layout_step_kernel does.
__global__ __launch_bounds__(kTile) void layout_batch_step_kernel(const uint2* __restrict__ tiles,
                                                                  const uint32_t* __restrict__ comp_off,
                                                                  const double* __restrict__ x_all,
                                                                  const double* __restrict__ y_all,
                                                                  double* __restrict__ x_out, double* __restrict__ y_out,
                                                                  const uint32_t* __restrict__ adj_off,
                                                                  const uint32_t* __restrict__ adj,
                                                                  const double* __restrict__ k_of, double t) {
    __shared__ double sx[kTile], sy[kTile];
    const uint2 tile = tiles[blockIdx.x];
    const uint32_t base = comp_off[tile.x], n = comp_off[tile.x + 1] - base;
    const double* __restrict__ x = x_all + base;
    const double* __restrict__ y = y_all + base;
    const double k = k_of[tile.x];
    const uint32_t i = tile.y + threadIdx.x;
    const double px = i < n ? x[i] : 0.0, py = i < n ? y[i] : 0.0;
    double ax = 0.0, ay = 0.0;
    for (uint32_t m0 = 0; m0 < n; m0 += kTile) {
        const uint32_t m = m0 + threadIdx.x;
        sx[threadIdx.x] = m < n ? x[m] : 0.0;
        sy[threadIdx.x] = m < n ? y[m] : 0.0;
        __syncthreads();
        const uint32_t cnt = n - m0 < (uint32_t)kTile ? n - m0 : (uint32_t)kTile;
        if (i < n) {
            for (uint32_t j = 0; j < cnt; ++j) {
                if (m0 + j == i) continue;
                const double dx = px - sx[j], dy = py - sy[j];
                double distance = sqrt(dx * dx + dy * dy);
                if (distance < 0.01) distance = 0.01;
                const double s = (k * k) / (distance * distance);
                ax = ax + dx * s;
                ay = ay + dy * s;
            }
        }
        __syncthreads();
    }
    if (i >= n) return;
    for (uint32_t a = adj_off[base + i]; a < adj_off[base + i + 1]; ++a) {
        const uint32_t m = adj[a];
        const double mx = m < n ? x[m] : 0.0, my = m < n ? y[m] : 0.0;     // index n: the origin
        const double dx = px - mx, dy = py - my;
        double distance = sqrt(dx * dx + dy * dy);
        if (distance < 0.01) distance = 0.01;
        const double s = -1. * distance / k;
        ax = ax + dx * s;
        ay = ay + dy * s;
    }
    double length = sqrt(ax * ax + ay * ay);
    if (length < 0.01) length = 0.1;                    // sic (graph.cpp:1208-1210)
    const double s = t / length;
    x_out[base + i] = px + ax * s;
    y_out[base + i] = py + ay * s;
}

}  // namespace

void launch_layout_step(uint32_t n, const double* x, const double* y, double* x_out, double* y_out,
                        const uint32_t* adj_off, const uint32_t* adj, double k, double t, hipStream_t s) {
    if (n) {
        hipLaunchKernelGGL(layout_step_kernel, dim3((n + kTile - 1) / kTile), dim3(kTile), 0, s, n, x, y, x_out, y_out,
                           adj_off, adj, k, t);
    }
}

void launch_layout_fused(uint32_t block, uint32_t n_list, const uint32_t* list, const uint32_t* comp_off, const double* x,
                         const double* y, double* x_out, double* y_out, const uint32_t* adj_off, const uint32_t* adj,
                         const double* k, uint32_t iterations, double t, double dt, hipStream_t s) {
    if (!n_list) return;
    if (block == 256) {
        hipLaunchKernelGGL(layout_fused_kernel<256>, dim3(n_list), dim3(256), 0, s, list, comp_off, x, y, x_out, y_out,
                           adj_off, adj, k, iterations, t, dt);
    } else {
        hipLaunchKernelGGL(layout_fused_kernel<1024>, dim3(n_list), dim3(1024), 0, s, list, comp_off, x, y, x_out, y_out,
                           adj_off, adj, k, iterations, t, dt);
    }
}

void launch_layout_batch_step(uint32_t n_tiles, const uint2* tiles, const uint32_t* comp_off, const double* x, const double* y,
                              double* x_out, double* y_out, const uint32_t* adj_off, const uint32_t* adj, const double* k,
                              double t, hipStream_t s) {
    if (n_tiles) {
        hipLaunchKernelGGL(layout_batch_step_kernel, dim3(n_tiles), dim3(kTile), 0, s, tiles, comp_off, x, y, x_out, y_out,
                           adj_off, adj, k, t);
    }
}

}  // namespace rala_hip
