// The layout step of Graph::postprocess (reference rvaser/rala src/graph.cpp:1132-1226) for a batch whose points are
// shared out over the ranks of a sharded run (rala_hip_mg_layout_batch, layout_shard.hip).  The arithmetic per point is that
// of layout_step_kernel (layout_kernels.hip), operation for operation: one ax / ay pair per point, repulsion over ascending
// j with j == i skipped, then the attraction list in order, the same clamps, FP64, no contraction (the library is built with
// -ffp-contract=off; sqrt and division are correctly rounded) - so a point's new position is the same bits whichever rank,
// kernel or launch computed it.
//
// What differs is where the positions lie: x and y of a point side by side (double2).  A rank's share of a step is then ONE
// contiguous block of bytes (what the ranks exchange after every step), and a partner is one 16-byte load.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rala_hip {

namespace {

constexpr int kTile = 256;
static_assert(kTile == (int)kLayoutTile, "the tile table of rala_hip_mg_layout_batch is built for this tile");

// One step of one point, written once.  `src` says where the component's n positions of the previous step are:
//   span()        how many of them one tile() shows (at least 1)
//   tile(m0)      points m0 .. m0 + span() - 1 (called by every thread of the workgroup: it may hold a barrier)
//   done()        the tile is read (called by every thread likewise)
//   point(m)      one of them, m < n (the attraction partners)
// A thread without a point (mine == false) walks the tiles with the others and returns p.
template <class Source>
__device__ __forceinline__ double2 layout_point_step(Source& src, bool mine, uint32_t i, uint32_t n, double2 p, double k,
                                                     double t, const uint32_t* __restrict__ adj, uint32_t a0, uint32_t a1) {
    const double px = p.x, py = p.y;
    double ax = 0.0, ay = 0.0;
    const uint32_t span = src.span();
    for (uint32_t m0 = 0; m0 < n; m0 += span) {
        const double2* tile = src.tile(m0);
        const uint32_t cnt = n - m0 < span ? n - m0 : span;
        if (mine) {
            for (uint32_t j = 0; j < cnt; ++j) {
                if (m0 + j == i) continue;
                const double2 q = tile[j];
                const double dx = px - q.x, dy = py - q.y;
                double distance = sqrt(dx * dx + dy * dy);
                if (distance < 0.01) distance = 0.01;
                const double s = (k * k) / (distance * distance);
                ax = ax + dx * s;
                ay = ay + dy * s;
            }
        }
        src.done();
    }
    if (!mine) return p;
    for (uint32_t a = a0; a < a1; ++a) {
        const uint32_t m = adj[a];
        double mx = 0.0, my = 0.0;                          // index n: the origin
        if (m < n) { const double2 q = src.point(m); mx = q.x; my = q.y; }
        const double dx = px - mx, dy = py - my;
        double distance = sqrt(dx * dx + dy * dy);
        if (distance < 0.01) distance = 0.01;
        const double s = -1. * distance / k;
        ax = ax + dx * s;
        ay = ay + dy * s;
    }
    double length = sqrt(ax * ax + ay * ay);
    if (length < 0.01) length = 0.1;                        // sic (graph.cpp:1208-1210)
    const double s = t / length;
    return make_double2(px + ax * s, py + ay * s);
}

// the component's points in global memory, streamed through an LDS tile of kTile points
struct StreamedSource {
    const double2* __restrict__ g;      // the component's first point
    double2* lds;
    uint32_t n;
    __device__ __forceinline__ uint32_t span() const { return (uint32_t)kTile; }
    __device__ __forceinline__ const double2* tile(uint32_t m0) {
        const uint32_t m = m0 + threadIdx.x;
        lds[threadIdx.x] = m < n ? g[m] : make_double2(0.0, 0.0);
        __syncthreads();
        return lds;
    }
    __device__ __forceinline__ void done() { __syncthreads(); }
    __device__ __forceinline__ double2 point(uint32_t m) const { return g[m]; }
};

// the component's points in LDS, all of them
struct ResidentSource {
    const double2* p;
    uint32_t n;
    __device__ __forceinline__ uint32_t span() const { return n; }
    __device__ __forceinline__ const double2* tile(uint32_t) { return p; }
    __device__ __forceinline__ void done() {}
    __device__ __forceinline__ double2 point(uint32_t m) const { return p[m]; }
};

// One step of the tiles tiles[0 .. gridDim.x) - a rank's range of the batch's tile table {component, first local point}: a
// workgroup reads its component's points of buffer `cur` and writes its own points of `out` (the other buffer), nothing else.
__global__ __launch_bounds__(kTile) void layout_shard_step_kernel(const uint2* __restrict__ tiles,
                                                                  const uint32_t* __restrict__ comp_off,
                                                                  const double2* __restrict__ cur, double2* __restrict__ out,
                                                                  const uint32_t* __restrict__ adj_off,
                                                                  const uint32_t* __restrict__ adj,
                                                                  const double* __restrict__ k_of, double t) {
    __shared__ double2 lds[kTile];
    const uint2 tile = tiles[blockIdx.x];
    const uint32_t base = comp_off[tile.x], n = comp_off[tile.x + 1] - base;
    const uint32_t i = tile.y + threadIdx.x;
    const bool mine = i < n;
    StreamedSource src{cur + base, lds, n};
    double2 p = make_double2(0.0, 0.0);
    uint32_t a0 = 0, a1 = 0;
    if (mine) { p = cur[base + i]; a0 = adj_off[base + i]; a1 = adj_off[base + i + 1]; }
    const double2 moved = layout_point_step(src, mine, i, n, p, k_of[tile.x], t, adj, a0, a1);
    if (mine) out[base + i] = moved;
}

// A component of at most BLOCK points: one workgroup, every step inside the launch (layout_fused_kernel's scheme).  The
// positions live in LDS, double-buffered; one barrier per step - a step reads buffer `cur` only and writes buffer `cur ^ 1`
// only, and nobody passes the barrier before everybody has finished reading.  The step length is t, t - dt, (t - dt) - dt, ...
// `out` may be `in`: a point is its thread's.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void layout_shard_fused_kernel(const uint32_t* __restrict__ list,
                                                                   const uint32_t* __restrict__ comp_off, const double2* in,
                                                                   double2* out, const uint32_t* __restrict__ adj_off,
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
    double2 p = make_double2(0.0, 0.0);
    if (mine) {
        p = in[base + i];
        a0 = adj_off[base + i]; a1 = adj_off[base + i + 1];
        pos[0][i] = p;
    }
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t it = 0; it < iterations; ++it) {
        ResidentSource src{pos[cur], n};
        p = layout_point_step(src, mine, i, n, p, k, t, adj, a0, a1);
        if (mine) pos[cur ^ 1][i] = p;
        __syncthreads();
        cur ^= 1;
        t -= dt;
    }
    if (mine) out[base + i] = p;
}

}  // namespace

void launch_layout_shard_step(uint32_t n_tiles, const uint2* tiles, const uint32_t* comp_off, const double2* cur, double2* out,
                              const uint32_t* adj_off, const uint32_t* adj, const double* k, double t, hipStream_t s) {
    if (n_tiles) {
        hipLaunchKernelGGL(layout_shard_step_kernel, dim3(n_tiles), dim3(kTile), 0, s, tiles, comp_off, cur, out, adj_off, adj,
                           k, t);
    }
}

void launch_layout_shard_fused(uint32_t block, uint32_t n_list, const uint32_t* list, const uint32_t* comp_off,
                               const double2* in, double2* out, const uint32_t* adj_off, const uint32_t* adj, const double* k,
                               uint32_t iterations, double t, double dt, hipStream_t s) {
    if (!n_list) return;
    if (block == 256) {
        hipLaunchKernelGGL(layout_shard_fused_kernel<256>, dim3(n_list), dim3(256), 0, s, list, comp_off, in, out, adj_off, adj,
                           k, iterations, t, dt);
    } else {
        hipLaunchKernelGGL(layout_shard_fused_kernel<1024>, dim3(n_list), dim3(1024), 0, s, list, comp_off, in, out, adj_off,
                           adj, k, iterations, t, dt);
    }
}

}  // namespace rala_hip
