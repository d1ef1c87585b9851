// rala_hip_mg_layout_batch: the force-directed layout of all components of a round (reference rvaser/rala
// src/graph.cpp:1132-1226, once per component of the loop at :1106), the POINTS shared out over the ranks of a sharded run.
// rala_hip_layout_batch (layout.hip) runs on one context while the other devices of `--gpus N` wait; its cost grows with the
// square of a component and its arithmetic is fixed (one accumulator pair per point, partners in ascending order), so more
// devices are the only direction left.  A step is a Jacobi step - a point's new position depends on the previous positions
// only - so any split of the points gives the same bits: every rank holds the whole batch, computes its own points of a step
// (layout_shard_kernels.hip) and the ranks all-gather the buffer just written, 16 bytes per point against n_c pair terms.
//
// Here: the split (rala_hip_layout_split, no device) and the three steps of the call (stages.h); the entry points and the
// host exchange between the steps are sharded.hip's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "ctx_check.h"
#include "stages.h"

using namespace rala_hip;

namespace {

size_t align_up(size_t bytes, size_t to) { return (bytes + to - 1) / to * to; }

double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the units of the split in point order: fn(one behind the unit's last point, its cost)
template <class Fn>
void for_each_unit(uint32_t n_components, const uint32_t* comp_off, uint32_t fused_max, Fn fn) {
    for (uint32_t c = 0; c < n_components; ++c) {
        const uint64_t base = comp_off[c], n_c = comp_off[c + 1] - comp_off[c];
        if (n_c == 0) continue;
        if (n_c <= fused_max) {
            fn((uint32_t)(base + n_c), n_c * n_c);
        } else {
            for (uint64_t first = 0; first < n_c; first += kLayoutTile) {
                const uint64_t points = n_c - first < kLayoutTile ? n_c - first : kLayoutTile;
                fn((uint32_t)(base + first + points), points * n_c);
            }
        }
    }
}

}  // namespace

int rala_hip_layout_split(uint32_t n_components, const uint32_t* comp_off, uint32_t fused_max, uint32_t parts, uint32_t* first_point,
                          uint64_t* cost) {
    if (parts == 0 || !first_point || (n_components && !comp_off) || fused_max > 1024) return RALA_HIP_EINVAL;
    if (n_components && comp_off[0] != 0) return RALA_HIP_EINVAL;
    for (uint32_t c = 0; c < n_components; ++c) {
        if (comp_off[c + 1] < comp_off[c]) return RALA_HIP_EINVAL;
    }
    const uint32_t N = n_components ? comp_off[n_components] : 0;
    // (the tiles of a component cost n_c^2 together; the sum is at most N^2 < 2^64)
    uint64_t total = 0;
    for (uint32_t c = 0; c < n_components; ++c) {
        const uint64_t n_c = comp_off[c + 1] - comp_off[c];
        total += n_c * n_c;
    }
    auto target = [&](uint32_t part) {
        const unsigned __int128 scaled = (unsigned __int128)total * ((uint64_t)part + 1);
        return (uint64_t)((scaled + parts - 1) / parts);
    };
    uint32_t part = 0;
    uint64_t prefix = 0, in_part = 0;
    first_point[0] = 0;
    for_each_unit(n_components, comp_off, fused_max, [&](uint32_t end, uint64_t unit) {
        prefix += unit;
        in_part += unit;
        // (a part whose target an earlier part's last unit has reached already ends where that one ended: it is empty)
        while (part + 1 < parts && prefix >= target(part)) {
            first_point[part + 1] = end;
            if (cost) cost[part] = in_part;
            in_part = 0;
            ++part;
        }
    });
    for (; part < parts; ++part) {
        first_point[part + 1] = N;
        if (cost) cost[part] = in_part;
        in_part = 0;
    }
    return RALA_HIP_OK;
}

namespace rala_hip {

int layout_shard_check(const LayoutShardBatch& b, const char** why) {
    auto refuse = [&](const char* what) { *why = what; return RALA_HIP_EINVAL; };
    const uint32_t C = b.n_components;
    if (C && !b.comp_off) return refuse("comp_off is null");
    if (C && b.comp_off[0] != 0) return refuse("comp_off does not start at 0");
    for (uint32_t c = 0; c < C; ++c) {
        if (b.comp_off[c + 1] < b.comp_off[c]) return refuse("comp_off decreases");
    }
    const size_t N = C ? b.comp_off[C] : 0;
    if (N && (!b.x || !b.y || !b.adj_off || !b.k)) return refuse("a null array");
    if (N && b.adj_off[0] != 0) return refuse("adj_off does not start at 0");
    for (size_t p = 0; p < N; ++p) {
        if (b.adj_off[p + 1] < b.adj_off[p]) return refuse("adj_off decreases");
    }
    const size_t A = N ? b.adj_off[N] : 0;
    if (A && !b.adj) return refuse("adj is null");
    for (uint32_t c = 0; c < C && N; ++c) {
        const uint32_t n_c = b.comp_off[c + 1] - b.comp_off[c];
        for (size_t a = b.adj_off[b.comp_off[c]]; a < b.adj_off[b.comp_off[c + 1]]; ++a) {
            if (b.adj[a] > n_c) return refuse("a partner index beyond its component");
        }
    }
    return RALA_HIP_OK;
}

int layout_shard_prepare(rala_hip_ctx* ctx, LayoutShardState& st, uint32_t rank, uint32_t world, const LayoutShardBatch& b) {
    const uint32_t C = b.n_components;
    const size_t N = C ? b.comp_off[C] : 0;
    const size_t A = N ? b.adj_off[N] : 0;
    const uint32_t fused_max = (uint32_t)ctx->layout_fused_max;
    st.first_point.assign((size_t)world + 1, 0);
    std::vector<uint64_t> cost(world, 0);
    if (rala_hip_layout_split(C, b.comp_off, fused_max, world, st.first_point.data(), cost.data()) != RALA_HIP_OK) {
        return fail(ctx, RALA_HIP_EINVAL, "rala_hip_mg_layout_batch: the split refused its input");
    }
    const uint32_t lo = st.first_point[rank], hi = st.first_point[rank + 1];
    // ---- which component takes which path, and what of it is this rank's (a cut lies on a unit's edge: a unit that begins in
    //      [lo, hi) lies in it) ----
    std::vector<uint32_t> list256, list1024, tiles;
    uint32_t own_first = 0, own_tiles = 0;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t base = b.comp_off[c], n_c = b.comp_off[c + 1] - base;
        if (n_c == 0) continue;
        const bool mine = base >= lo && base < hi;
        if (n_c <= fused_max) {
            if (mine) (n_c <= 256 ? list256 : list1024).push_back(c);
        } else {
            for (uint32_t first = 0; first < n_c; first += kLayoutTile) {
                if (base + first >= lo && base + first < hi) {
                    if (!own_tiles) own_first = (uint32_t)(tiles.size() / 2);
                    ++own_tiles;
                }
                tiles.push_back(c); tiles.push_back(first);
            }
        }
    }
    const size_t T = tiles.size() / 2;
    if (T > 0x7FFFFFFFull) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_mg_layout_batch: too many points for one launch");
    rala_hip_mg_layout_info info = {};
    info.first_point = lo; info.end_point = hi;
    info.components_fused_256 = (uint32_t)list256.size();
    info.components_fused_1024 = (uint32_t)list1024.size();
    info.step_tiles = own_tiles;
    info.cost = cost[rank];
    for (uint32_t p = 0; p < world; ++p) info.total_cost += cost[p];
    st.n_list256 = (uint32_t)list256.size(); st.n_list1024 = (uint32_t)list1024.size();
    st.tile_first = own_first; st.n_tiles_all = (uint32_t)T;
    if (N == 0 || b.iterations == 0) {
        st.info = info;
        return RALA_HIP_OK;
    }
    info.launches = (list256.empty() ? 0u : 1u) + (list1024.empty() ? 0u : 1u) + (own_tiles ? b.iterations : 0u);
    info.gathers = T ? b.iterations : 1u;
    info.bytes_received = (uint64_t)info.gathers * (N - (hi - lo)) * sizeof(double2);

    // ---- one block: [positions as {x, y} | k] doubles, [comp_off | adj_off | adj | list256 | list1024 | pad | tiles] words: the
    //      upload; behind it the second position buffer ----
    st.o_k = N * 16; st.o_comp = st.o_k + (size_t)C * 8;
    st.o_adj_off = st.o_comp + ((size_t)C + 1) * 4; st.o_adj = st.o_adj_off + (N + 1) * 4; st.o_l256 = st.o_adj + A * 4;
    st.o_l1024 = st.o_l256 + list256.size() * 4; st.o_tiles = align_up(st.o_l1024 + list1024.size() * 4, 8);
    const size_t upload = st.o_tiles + T * 8;
    st.o_pos1 = align_up(upload, 16);
    HIPCHECK(hipSetDevice(ctx->device));
    for (auto& e : st.ev) if (!e) HIPCHECK(hipEventCreate(&e));
    HIPCHECK(st.d_block.ensure(st.o_pos1 + N * 16));
    HIPCHECK(st.p_block.ensure(upload));
    unsigned char* const h = st.p_block.p;
    double* const pos = (double*)h;
    for (size_t p = 0; p < N; ++p) { pos[2 * p] = b.x[p]; pos[2 * p + 1] = b.y[p]; }
    memcpy(h + st.o_k, b.k, (size_t)C * 8);
    memcpy(h + st.o_comp, b.comp_off, ((size_t)C + 1) * 4);
    memcpy(h + st.o_adj_off, b.adj_off, (N + 1) * 4);
    if (A) memcpy(h + st.o_adj, b.adj, A * 4);
    if (!list256.empty()) memcpy(h + st.o_l256, list256.data(), list256.size() * 4);
    if (!list1024.empty()) memcpy(h + st.o_l1024, list1024.data(), list1024.size() * 4);
    if (st.o_tiles > st.o_l1024 + list1024.size() * 4) memset(h + st.o_l1024 + list1024.size() * 4, 0, st.o_tiles - (st.o_l1024 + list1024.size() * 4));
    if (T) memcpy(h + st.o_tiles, tiles.data(), T * 8);
    HIPCHECK(hipMemcpyAsync(st.d_block.p, h, upload, hipMemcpyHostToDevice, ctx->stream));
    st.info = info;
    return RALA_HIP_OK;
}

int layout_shard_steps(rala_hip_ctx* ctx, Comm* comm, LayoutShardState& st, const LayoutShardBatch& b, double* x_out, double* y_out) {
    const uint32_t C = b.n_components, world = comm->world(), rank = comm->rank();
    const size_t N = C ? b.comp_off[C] : 0;
    if (N == 0 || b.iterations == 0) return RALA_HIP_OK;
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned char* const d = st.d_block.p;
    double2* const pos[2] = {(double2*)d, (double2*)(d + st.o_pos1)};
    const double* const d_k = (const double*)(d + st.o_k);
    const uint32_t* const d_comp = (const uint32_t*)(d + st.o_comp);
    const uint32_t* const d_adj_off = (const uint32_t*)(d + st.o_adj_off);
    const uint32_t* const d_adj = (const uint32_t*)(d + st.o_adj);
    const uint2* const d_tiles = (const uint2*)(d + st.o_tiles) + st.tile_first;
    std::vector<uint64_t> counts(world);
    for (uint32_t p = 0; p < world; ++p) counts[p] = st.first_point[p + 1] - st.first_point[p];
    const uint32_t lo = st.first_point[rank];
    float device_ms = 0;
    double exchange_ms = 0;
    // the kernels enqueued since ev[0] are done (their time is added up), then the ranks' point ranges of `buffer` travel: the
    // rank's own range is where it is, the others' arrive beside it
    auto gather = [&](int buffer) {
        HIPCHECK(hipEventRecord(st.ev[1], s));
        HIPCHECK(hipEventSynchronize(st.ev[1]));
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, st.ev[0], st.ev[1]));
        device_ms += ms;
        const double t0 = wall_ms();
        const int rc = comm->all_gather_v(pos[buffer] + lo, pos[buffer], counts.data(), sizeof(double2), s);
        exchange_ms += wall_ms() - t0;
        if (rc != 0) return fail(ctx, RALA_HIP_EDEVICE, "rala_hip_mg_layout_batch: all-gather of the positions: " + comm->error());
        return (int)RALA_HIP_OK;
    };
    // where the stepped components end up after `iterations` swaps; the fused ones write there directly
    const int last = (int)(b.iterations & 1u);
    HIPCHECK(hipEventRecord(st.ev[0], s));
    launch_layout_shard_fused(256, st.n_list256, (const uint32_t*)(d + st.o_l256), d_comp, pos[0], pos[last], d_adj_off, d_adj, d_k,
                              b.iterations, b.t, b.dt, s);
    launch_layout_shard_fused(1024, st.n_list1024, (const uint32_t*)(d + st.o_l1024), d_comp, pos[0], pos[last], d_adj_off, d_adj,
                              d_k, b.iterations, b.t, b.dt, s);
    if (st.n_tiles_all) {
        int cur = 0;
        double t_step = b.t;
        for (uint32_t it = 0; it < b.iterations; ++it) {
            if (it) HIPCHECK(hipEventRecord(st.ev[0], s));
            launch_layout_shard_step(st.info.step_tiles, d_tiles, d_comp, pos[cur], pos[cur ^ 1], d_adj_off, d_adj, d_k, t_step, s);
            // (the last one is no special case: a rank's own range of the result buffer is only ever written by that rank, so it
            // carries the fused results as well)
            const int rc = gather(cur ^ 1);
            if (rc != RALA_HIP_OK) return rc;
            cur ^= 1;
            t_step -= b.dt;
        }
    } else {
        const int rc = gather(last);
        if (rc != RALA_HIP_OK) return rc;
    }
    HIPCHECK(hipGetLastError());
    if (x_out || y_out) {
        // x and y of a point lie side by side: one copy (into the pinned block, which the upload has left by now)
        double* const h = (double*)st.p_block.p;
        HIPCHECK(hipMemcpyAsync(h, pos[last], N * 16, hipMemcpyDeviceToHost, s));
        HIPCHECK(stream_sync(ctx, s));
        if (x_out) for (size_t p = 0; p < N; ++p) x_out[p] = h[2 * p];
        if (y_out) for (size_t p = 0; p < N; ++p) y_out[p] = h[2 * p + 1];
    } else {
        HIPCHECK(stream_sync(ctx, s));
    }
    st.info.device_ms = device_ms;
    st.info.exchange_ms = (float)exchange_ms;
    return RALA_HIP_OK;
}

void layout_shard_release(LayoutShardState& st) {
    for (auto& e : st.ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    st.d_block.release();
    st.p_block.release();
}

}  // namespace rala_hip
