// librala_hip: Graph::remove_transitive_edges.  Implements rala_hip_remove_transitive_edges and rala_hip_tr_mark of
// rala_hip.h and transitive_stage of stages.h.
#include <hip/hip_runtime.h>

#include "lifecycle.h"
#include "orchestration.h"
#include "scan_pass.h"

using namespace rala_hip;

namespace {

// transitive-edge marking on device edge arrays; marks stay in ctx->d_tr_marks
int tr_mark_device(rala_hip_ctx* ctx, uint32_t n_nodes, uint32_t n_edges, const uint32_t* d_src, const uint32_t* d_dst,
                   const uint32_t* d_len, uint32_t* n_pairs, Comm* comm = nullptr) {
    *n_pairs = 0;
    if (n_edges == 0) return RALA_HIP_OK;
    if (n_edges & 1) return fail(ctx, RALA_HIP_EINVAL, "edges must come in twin pairs (e, e^1)");
    hipStream_t s = ctx->stream;
    DevBuf<uint32_t>* B = ctx->d_tr;          // row, cursor, adj (persistent)
    HIPCHECK(B[0].ensure(n_nodes + 2)); HIPCHECK(B[1].ensure(n_nodes + 2)); HIPCHECK(B[2].ensure(2 * (size_t)n_edges));
    HIPCHECK(ctx->d_tr_marks.ensure((size_t)n_edges + 8));
    HIPCHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes((uint64_t)n_nodes + 2)));
    HIPCHECK(hipEventRecord(ctx->ev[kEvTrBegin], s));
    FillList fills;
    fills.add(ctx->d_tr_marks.p, 0, ((size_t)n_edges + 7) & ~(size_t)3);
    fills.add(ctx->d_small.p + kTrBadEndpoint, 0, kTrWords * 4);     // (the bad-endpoint flag and the pairs)
    fills.add(B[1].p, 0, (size_t)(n_nodes + 1) * 4);
    // CSR on the device: out-degree count -> scan -> fill.  The fill order is arbitrary; the
    // candidate a->c is the edge with the highest id, which is the reference's "last one
    // in suffix_edges_" (graph.cpp:1291-1293, out-lists are in edge-id order there).
    ScanSpace sp;
    {
        const int rc = scan_space(ctx, 1, n_nodes, sp, &fills);
        if (rc != RALA_HIP_OK) return rc;
    }
    HIPCHECK(fills.launch(s));
    launch_tr_degree(d_src, d_dst, n_nodes, n_edges, B[1].p, ctx->d_small.p + kTrBadEndpoint, s);
    // row offsets (and the fill cursors, a second copy of them) from the out-degrees: one launch
    HIPCHECK(B[3 + 3].ensure(n_nodes + 2));
    if (!launch_offsets_pass(B[1].p, B[0].p, B[6].p, n_nodes, sp, s)) return fail(ctx, RALA_HIP_EDEVICE, "scan space");
    launch_tr_fill(d_src, d_dst, n_nodes, n_edges, B[6].p, B[2].p, s);
    if (!comm) {
        launch_tr_mark(B[0].p, B[2].p, d_src, d_dst, d_len, n_nodes, 0, n_edges, ctx->d_tr_marks.p, s);
    } else {
        // every rank probes from its share of the edges a->b; the marks (bytes 0 / 1) are summed
        const uint64_t P = comm->world(), k = comm->rank();
        launch_tr_mark(B[0].p, B[2].p, d_src, d_dst, d_len, n_nodes, (uint32_t)(n_edges * k / P), (uint32_t)(n_edges * (k + 1) / P),
                       ctx->d_tr_marks.p, s);
        if (comm->all_reduce_u32((uint32_t*)ctx->d_tr_marks.p, ((size_t)n_edges + 3) / 4, ReduceOp::kSum, s) != 0) {
            ctx->err = std::string("all-reduce of the transitive marks: ") + comm->error();
            return RALA_HIP_EDEVICE;
        }
    }
    launch_tr_count(ctx->d_tr_marks.p, n_edges, ctx->d_small.p + kTrPairs, s);
    HIPCHECK(hipEventRecord(ctx->ev[kEvTrEnd], s));
    uint32_t res[kTrWords] = {};
    HIPCHECK(d2h_small(ctx, res, ctx->d_small.p + kTrBadEndpoint, sizeof(res), s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventElapsedTime(&ctx->tm.tr_ms, ctx->ev[kEvTrBegin], ctx->ev[kEvTrEnd]));
    if (res[kTrBadEndpoint - kTrBadEndpoint]) return fail(ctx, RALA_HIP_EINVAL, "edge endpoint out of range");
    *n_pairs = res[kTrPairs - kTrBadEndpoint];
    return RALA_HIP_OK;
}

int tr_mark_impl(rala_hip_ctx* ctx, uint32_t n_nodes, uint32_t n_edges, const uint32_t* src, const uint32_t* dst,
                 const uint32_t* len, uint8_t* marks, uint32_t* n_pairs) {
    *n_pairs = 0;
    if (n_edges == 0) return RALA_HIP_OK;
    hipStream_t s = ctx->stream;
    DevBuf<uint32_t>* B = ctx->d_tr;
    HIPCHECK(B[3].ensure(n_edges)); HIPCHECK(B[4].ensure(n_edges)); HIPCHECK(B[5].ensure(n_edges));
    HIPCHECK(hipMemcpyAsync(B[3].p, src, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(B[4].p, dst, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(B[5].p, len, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
    const int rc = tr_mark_device(ctx, n_nodes, n_edges, B[3].p, B[4].p, B[5].p, n_pairs);
    if (rc != RALA_HIP_OK) return rc;
    HIPCHECK(hipMemcpy(marks, ctx->d_tr_marks.p, n_edges, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

}  // namespace

int rala_hip::transitive_stage(rala_hip_ctx* ctx, Comm* comm, uint32_t* n_pairs) {
    if (!ctx || !n_pairs) return RALA_HIP_EINVAL;
    if (!ctx->constructed) return fail(ctx, RALA_HIP_EINVAL, "construct must succeed first");
    HIPCHECK(hipSetDevice(ctx->device));
    if (ctx->tail_on_device) {
        const int rc = tr_mark_device(ctx, ctx->t_n_nodes, ctx->t_n_edges, ctx->d_e[0].p, ctx->d_e[1].p, ctx->d_e[2].p, n_pairs, comm);
        marks_left_on_device(ctx, rc == RALA_HIP_OK);
        return rc;
    }
    // (the tail ran on the host, or the sensitive pass rebuilt the graph there: a host graph)
    const uint32_t ne = (uint32_t)ctx->e_src.size();
    ctx->e_mark.assign(ne, 0);
    return tr_mark_impl(ctx, (uint32_t)ctx->node_read.size(), ne, ctx->e_src.data(), ctx->e_dst.data(),
                        ctx->e_len.data(), ctx->e_mark.data(), n_pairs);
}

extern "C" {

int rala_hip_remove_transitive_edges(rala_hip_ctx* ctx, uint32_t* n_pairs) {
    if (!ctx || !n_pairs) return RALA_HIP_EINVAL;
    if (!ctx->constructed) return fail(ctx, RALA_HIP_EINVAL, "rala_hip_construct must succeed first");
    return transitive_stage(ctx, nullptr, n_pairs);
}

int rala_hip_tr_mark(rala_hip_ctx* ctx, uint32_t n_nodes, uint32_t n_edges, const uint32_t* src,
                     const uint32_t* dst, const uint32_t* len, uint8_t* marks, uint32_t* n_pairs) {
    if (!ctx || !n_pairs || (n_edges && (!src || !dst || !len || !marks))) return RALA_HIP_EINVAL;
    HIPCHECK(hipSetDevice(ctx->device));
    return tr_mark_impl(ctx, n_nodes, n_edges, src, dst, len, marks, n_pairs);
}

}  // extern "C"
