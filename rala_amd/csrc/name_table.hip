// Host side of the name table built on the device (name_table_kernels.hip): build from the context's sequence index, read back,
// copy from context to context.  rala_hip_set_name_table (ingest.hip) installs a table the host built; these install, read and
// copy the same two buffers (d_name_buckets, d_name_arena).
#include "ingest_common.h"
#include "name_table.h"

using namespace rala_hip;
using namespace rala_hip::ingest;

namespace {

template <class T>
void swap_buffers(DevBuf<T>& a, DevBuf<T>& b) {         // (plain hipMalloc buffers: no chunks)
    std::swap(a.p, b.p);
    std::swap(a.n, b.n);
}

}  // namespace

extern "C" {

int rala_hip_build_name_table(rala_hip_ctx* ctx, uint64_t* n_buckets, uint64_t* n_distinct) {
    if (!ctx || !n_buckets || !n_distinct) return RALA_HIP_EINVAL;
    *n_buckets = *n_distinct = 0;
    if (!ctx->seq_index_valid) return fail(ctx, RALA_HIP_EINVAL, "no sequence index (rala_hip_index_sequences)");
    const uint64_t n = ctx->n_seq_records, bytes = ctx->n_seq_name_bytes;
    if (bytes >= (1ull << 32)) return fail(ctx, RALA_HIP_ETOOLARGE, "2^32 bytes of names or more: a bucket's offset has 32 bits");
    if (n >= 0xFFFFFFFFull) return fail(ctx, RALA_HIP_ETOOLARGE, "2^32 - 1 records or more: a bucket holds id + 1 in 32 bits");
    uint64_t cap = 16;
    while (cap < 2 * n + 2) cap <<= 1;                  // (NameTable::build's rule)
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (auto& e : ctx->ev_names) if (!e) HIPCHECK(hipEventCreate(&e));
    // built beside the installed table, which stays as it is until this one is whole
    DevBuf<uint8_t> buckets, arena;
    HIPCHECK(buckets.ensure(cap * sizeof(NameBucket)));
    HIPCHECK(arena.ensure(bytes + 16));
    HIPCHECK(ctx->d_name_stats.ensure(4));
    HIPCHECK(hipEventRecord(ctx->ev_names[0], s));
    HIPCHECK(hipMemsetAsync(buckets.p, 0, cap * sizeof(NameBucket), s));
    HIPCHECK(hipMemsetAsync(ctx->d_name_stats.p, 0, 16, s));
    launch_name_table_build(ctx->d_seq_arena.p, ctx->d_seq_name_off.p, ctx->d_seq_name_len.p, (uint32_t)n, buckets.p, cap, ctx->d_name_stats.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemsetAsync(arena.p + bytes, 0, 16, s));
    if (bytes) HIPCHECK(hipMemcpyAsync(arena.p, ctx->d_seq_arena.p, bytes, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipEventRecord(ctx->ev_names[1], s));
    uint32_t stats[4] = {0, 0, 0, 0};
    HIPCHECK(hipMemcpyAsync(stats, ctx->d_name_stats.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (stats[0]) return fail(ctx, RALA_HIP_EDEVICE, "the name table's build did not end within its bound (a probe path of n_buckets slots)");
    rala_hip_name_table_info info = {};
    HIPCHECK(hipEventElapsedTime(&info.device_ms, ctx->ev_names[0], ctx->ev_names[1]));
    info.names = n;
    info.distinct = stats[2];
    info.n_buckets = cap;
    info.longest_probe = stats[1];
    swap_buffers(ctx->d_name_buckets, buckets);
    swap_buffers(ctx->d_name_arena, arena);
    ctx->n_name_buckets = cap;
    ctx->n_name_arena_bytes = bytes;
    ctx->name_table_info = info;
    if (trace_on()) {
        fprintf(stderr, "[trace] device name table: %lu names, %lu distinct, in %lu buckets in %.3f ms (longest probe path %u slots)\n",
                (unsigned long)n, (unsigned long)info.distinct, (unsigned long)cap, info.device_ms, info.longest_probe);
    }
    *n_buckets = cap;
    *n_distinct = stats[2];
    return RALA_HIP_OK;
}

int rala_hip_get_name_table(rala_hip_ctx* ctx, void* buckets, char* arena, uint64_t* n_buckets, uint64_t* arena_bytes) {
    if (!ctx || !n_buckets || !arena_bytes) return RALA_HIP_EINVAL;
    *n_buckets = *arena_bytes = 0;
    if (ctx->n_name_buckets == 0) return fail(ctx, RALA_HIP_EINVAL, "no name table set");
    *n_buckets = ctx->n_name_buckets;
    *arena_bytes = ctx->n_name_arena_bytes;
    if (!buckets && !arena) return RALA_HIP_OK;
    HIPCHECK(hipSetDevice(ctx->device));
    if (buckets) HIPCHECK(hipMemcpy(buckets, ctx->d_name_buckets.p, ctx->n_name_buckets * sizeof(NameBucket), hipMemcpyDeviceToHost));
    if (arena && ctx->n_name_arena_bytes) HIPCHECK(hipMemcpy(arena, ctx->d_name_arena.p, ctx->n_name_arena_bytes, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

int rala_hip_copy_name_table(rala_hip_ctx* dst, rala_hip_ctx* src) {
    if (!dst || !src) return RALA_HIP_EINVAL;
    rala_hip_ctx* ctx = dst;                            // (HIPCHECK's)
    if (src->n_name_buckets == 0) return fail(ctx, RALA_HIP_EINVAL, "no name table set on the source");
    if (dst == src) return RALA_HIP_OK;
    const size_t table_bytes = src->n_name_buckets * sizeof(NameBucket), arena_bytes = src->n_name_arena_bytes + 16;
    HIPCHECK(hipSetDevice(src->device));
    HIPCHECK(hipStreamSynchronize(src->stream));
    HIPCHECK(hipSetDevice(dst->device));
    // (a table of another size: made beside the old one, which a failure leaves installed)
    DevBuf<uint8_t> buckets, arena;
    HIPCHECK(buckets.ensure(table_bytes));
    HIPCHECK(arena.ensure(arena_bytes));
    int peer = 1;
    if (dst->device != src->device) HIPCHECK(hipDeviceCanAccessPeer(&peer, dst->device, src->device));
    const struct { uint8_t* to; const uint8_t* from; size_t bytes; } part[2] = {{buckets.p, src->d_name_buckets.p, table_bytes},
                                                                                 {arena.p, src->d_name_arena.p, arena_bytes}};
    if (dst->device == src->device) {
        for (const auto& p : part) HIPCHECK(hipMemcpy(p.to, p.from, p.bytes, hipMemcpyDeviceToDevice));
    } else if (peer) {
        for (const auto& p : part) HIPCHECK(hipMemcpyPeer(p.to, dst->device, p.from, src->device, p.bytes));
    } else {
        PinnedBuf<uint8_t> stage;
        HIPCHECK(stage.ensure(kBlockBytes));
        for (const auto& p : part) {
            for (size_t at = 0; at < p.bytes; at += kBlockBytes) {
                const size_t take = std::min(kBlockBytes, p.bytes - at);
                HIPCHECK(hipSetDevice(src->device));
                HIPCHECK(hipMemcpy(stage.p, p.from + at, take, hipMemcpyDeviceToHost));
                HIPCHECK(hipSetDevice(dst->device));
                HIPCHECK(hipMemcpy(p.to + at, stage.p, take, hipMemcpyHostToDevice));
            }
        }
    }
    HIPCHECK(hipStreamSynchronize(dst->stream));    // (nothing of dst's still reads the table it had)
    swap_buffers(dst->d_name_buckets, buckets);
    swap_buffers(dst->d_name_arena, arena);
    dst->n_name_buckets = src->n_name_buckets;
    dst->n_name_arena_bytes = src->n_name_arena_bytes;
    return RALA_HIP_OK;
}

uint64_t rala_hip_name_hash(const char* p, uint64_t n) {
    return name_hash_with(n, [p](uint64_t k, uint64_t m) {
        uint64_t w = 0;
        memcpy(&w, p + k, (size_t)m);
        return w;
    });
}

int rala_hip_get_name_table_info(rala_hip_ctx* ctx, rala_hip_name_table_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->name_table_info;
    return RALA_HIP_OK;
}

}  // extern "C"
