// Node bases as spans (include/rala_hip.h): the context's table of bases, and rala_hip_spell - the bytes that a list of spans
// of it spells, written by spell_kernels.hip and brought to the host window by window.
#include <algorithm>
#include <vector>

#include "ingest_common.h"
#include "spell.h"

using namespace rala_hip;

void rala_hip::bases_released(rala_hip_ctx* ctx) {
    ctx->d_bases.release();
    ctx->d_base_off.release();
    ctx->h_base_off.clear();
    ctx->n_base_sources = 0;
    ctx->bases_from_slice = false;
    ctx->spell_info.sources = ctx->spell_info.source_bytes = 0;
    ctx->spell_info.from_slice = 0;
}

int rala_hip::bases_adopted(rala_hip_ctx* ctx, const uint64_t* base_off, uint64_t n_sources, bool from_slice) {
    if (ctx->d_base_off.ensure(n_sources + 1) != hipSuccess) {
        bases_released(ctx);
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the offsets of the table of bases");
    }
    if (hipMemcpy(ctx->d_base_off.p, base_off, (n_sources + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) {
        bases_released(ctx);
        return fail(ctx, RALA_HIP_EDEVICE, "copying the offsets of the table of bases failed");
    }
    ctx->h_base_off.assign(base_off, base_off + n_sources + 1);
    ctx->n_base_sources = n_sources;
    ctx->bases_from_slice = from_slice;
    ctx->spell_info.sources = n_sources;
    ctx->spell_info.source_bytes = base_off[n_sources];
    ctx->spell_info.from_slice = from_slice ? 1u : 0u;
    return RALA_HIP_OK;
}

extern "C" {

int rala_hip_set_bases(rala_hip_ctx* ctx, const uint8_t* bases, const uint64_t* base_off, uint64_t n_sources, int mem) {
    if (!ctx || (n_sources && !base_off) || (mem != RALA_HIP_MEM_HOST && mem != RALA_HIP_MEM_DEVICE)) return RALA_HIP_EINVAL;
    if (n_sources > (1ull << 32)) return fail(ctx, RALA_HIP_ETOOLARGE, "more sources than a span's 32 bits name");
    HIPCHECK(hipSetDevice(ctx->device));
    if (!n_sources) {
        bases_released(ctx);
        return RALA_HIP_OK;
    }
    if (base_off[0] != 0) return fail(ctx, RALA_HIP_EINVAL, "base_off does not begin at 0");
    for (uint64_t s = 0; s < n_sources; ++s) {
        if (base_off[s + 1] < base_off[s]) return fail(ctx, RALA_HIP_EINVAL, "base_off decreases");
    }
    const uint64_t bytes = base_off[n_sources];
    if (bytes && !bases) return RALA_HIP_EINVAL;
    bases_released(ctx);                        // (the old table goes first: both need not fit side by side)
    if (ctx->d_bases.ensure(bytes) != hipSuccess) {
        bases_released(ctx);
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the table of bases");
    }
    if (bytes && hipMemcpy(ctx->d_bases.p, bases, bytes, mem == RALA_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) != hipSuccess) {
        bases_released(ctx);
        return fail(ctx, RALA_HIP_EDEVICE, "copying the table of bases failed");
    }
    return bases_adopted(ctx, base_off, n_sources, false);
}

int rala_hip_spell(rala_hip_ctx* ctx, const rala_hip_span* spans, uint64_t n_spans, uint8_t* out, uint64_t out_bytes) {
    if (!ctx || (n_spans && !spans) || (out_bytes && !out)) return RALA_HIP_EINVAL;
    if (n_spans >= (1ull << 32)) return fail(ctx, RALA_HIP_ETOOLARGE, "2^32 spans or more");
    // everything is checked here, and the output offsets are formed in the same pass: a refused call has enqueued nothing
    if (ctx->h_base_off.empty()) return fail(ctx, RALA_HIP_EINVAL, "no table of bases (rala_hip_set_bases)");
    std::vector<uint64_t> off(n_spans + 1);
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_spans; ++k) {
        const rala_hip_span& s = spans[k];
        if (s.source >= ctx->n_base_sources) return fail(ctx, RALA_HIP_EINVAL, "a span of a source the table does not have");
        if ((uint64_t)s.first + s.len > ctx->h_base_off[s.source + 1] - ctx->h_base_off[s.source]) {
            return fail(ctx, RALA_HIP_EINVAL, "a span that ends beyond its source");
        }
        if (s.rc > 1) return fail(ctx, RALA_HIP_EINVAL, "a span whose rc is neither 0 nor 1");
        off[k] = total;
        total += s.len;
    }
    off[n_spans] = total;
    if (total != out_bytes) return fail(ctx, RALA_HIP_EINVAL, "the spans' lengths do not sum to out_bytes");
    rala_hip_spell_info& info = ctx->spell_info;
    info.spans = n_spans;
    info.bytes = info.windows = info.launches = 0;
    info.upload_ms = info.kernel_ms = info.copy_ms = 0;
    if (!n_spans || !out_bytes) return RALA_HIP_OK;
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t tile = spell_tile_bytes();
    uint64_t window = ctx->debug_spell_window ? (uint64_t)ctx->debug_spell_window : (uint64_t)std::max(1u, ctx->spell_window_mb) << 20;
    window = std::max(tile, window / tile * tile);
    // (this call's buffers do not stay the context's: a window is a quarter of a gigabyte, the spans of a large graph more)
    struct Release {
        rala_hip_ctx* ctx;
        ~Release() {
            ctx->d_spell_out.release();
            ctx->d_spell_spans.release();
            ctx->d_spell_off.release();
        }
    } release{ctx};
    const double t0 = now_ms();
    HIPCHECK(ctx->d_spell_spans.ensure(n_spans));
    HIPCHECK(ctx->d_spell_off.ensure(n_spans + 1));
    HIPCHECK(ctx->d_spell_out.ensure(std::min(window, (total + tile - 1) / tile * tile)));
    HIPCHECK(hipMemcpyAsync(ctx->d_spell_spans.p, spans, n_spans * sizeof(rala_hip_span), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_spell_off.p, off.data(), (n_spans + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    double kernel_ms = 0, copy_ms = 0;
    const double t1 = now_ms();
    for (uint64_t lo = 0; lo < total; lo += window) {
        SpellArgs A;
        A.bases = ctx->d_bases.p; A.base_off = ctx->d_base_off.p;
        A.spans = ctx->d_spell_spans.p; A.out_off = ctx->d_spell_off.p; A.n_spans = (uint32_t)n_spans;
        A.lo = lo; A.hi = std::min(total, lo + window);
        A.out = ctx->d_spell_out.p;
        const double tk = now_ms();
        launch_spell(A, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
        const double tc = now_ms();
        HIPCHECK(hipMemcpy(out + lo, ctx->d_spell_out.p, A.hi - lo, hipMemcpyDeviceToHost));
        kernel_ms += tc - tk;
        copy_ms += now_ms() - tc;
        ++info.windows;
        ++info.launches;
        info.bytes += A.hi - lo;
    }
    info.upload_ms = (float)(t1 - t0);
    info.kernel_ms = (float)kernel_ms;
    info.copy_ms = (float)copy_ms;
    if (trace_on()) {
        fprintf(stderr, "[trace] device spell: %lu spans, %lu bytes in %lu windows, upload %.2f ms, kernel %.2f ms, bytes to the host %.2f ms\n",
                (unsigned long)n_spans, (unsigned long)total, (unsigned long)info.windows, info.upload_ms, info.kernel_ms, info.copy_ms);
    }
    return RALA_HIP_OK;
}

int rala_hip_get_spell_info(rala_hip_ctx* ctx, rala_hip_spell_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->spell_info;
    return RALA_HIP_OK;
}

}  // extern "C"
