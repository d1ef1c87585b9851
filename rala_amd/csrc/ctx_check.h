// How an entry point of librala_hip leaves with an error: fail() and HIPCHECK, for every file that works on a rala_hip_ctx
// (the sharded runner's MGCHECK / mg_fail work on a rala_hip_mg and live in sharded.hip).
#pragma once

#include <string>

#include "context.h"

namespace rala_hip {

// Every error return drops the staged device -> host copies that were queued but not delivered yet (d2h_small, stages.h):
// their destinations are mostly locals of the function that is returning.
inline int fail(rala_hip_ctx* ctx, int code, const std::string& msg) {
    ctx->err = msg;
    ctx->stage_pending.clear();
    ctx->stage_used = 0;
    return code;
}

}  // namespace rala_hip

// (wants a rala_hip_ctx* named ctx in scope)
#define HIPCHECK(call)                                                                                                  \
    do {                                                                                                                \
        const hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) {                                                                                         \
            return rala_hip::fail(ctx, e_ == hipErrorOutOfMemory ? RALA_HIP_ENOMEM : RALA_HIP_EDEVICE,                  \
                                  std::string(#call) + ": " + hipGetErrorString(e_));                                   \
        }                                                                                                               \
    } while (0)
