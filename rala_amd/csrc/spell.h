// The context's table of bases (spell.hip), for the one other file that fills it: rala_hip_slice_sequences with the option
// keep_bases gathers straight into ctx->d_bases and then adopts its offsets.
#pragma once

#include "context.h"

namespace rala_hip {

// no table from here on
void bases_released(rala_hip_ctx* ctx);
// ctx->d_bases holds base_off[n_sources] bytes: the offsets (host memory) are checked nowhere else, kept on the host and
// uploaded; a failure leaves no table
int bases_adopted(rala_hip_ctx* ctx, const uint64_t* base_off, uint64_t n_sources, bool from_slice);

}  // namespace rala_hip
