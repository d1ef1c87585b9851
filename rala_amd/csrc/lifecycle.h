// The life of a rala_hip_ctx as named transitions: what the context holds (which inputs, which stage, where the results
// lie) is a set of flags in context.h, and these functions are the only code that assigns them.  Plain host code, no HIP
// calls.  Every entry point of the C ABI is gated on the flags (the table: DESIGN.md, "The life of a context"); what a
// transition means for a caller is said at the transition.
#pragma once

#include "context.h"

namespace rala_hip {

enum class Inputs { kOverlaps, kTuples, kRecords, kBlocks };

// ---- results ---------------------------------------------------------------------------------------------------------

// Nothing computed is the context's any more: every stage has to run again, no getter of per-read state, lists or graph
// answers.  What a setter, a new rala_hip_initialize and an installed state all need first.
// Two things stay, because a caller can see them: n_prefiltered (rala_hip_get_num_prefiltered answers in every state), and
// the repeat hills of the last sensitive construct or rala_hip_find_repetitive_hills - rala_hip_get_intervals(2) and
// rala_hip_find_repetitive_hills take them up again after the next rala_hip_initialize, until rala_hip_construct drops them
// (construct_begun).
inline void results_dropped(rala_hip_ctx* ctx) {
    ctx->initialized = ctx->constructed = false;
    ctx->piles_resident = ctx->ev_ready = ctx->ev_fixed = false;
    ctx->rowless = false;
    ctx->sens_csr_ready = false;
    ctx->tail_on_device = ctx->host_stale = ctx->marks_on_device = false;
    ctx->host_state_fresh = false;
}

// ---- inputs ----------------------------------------------------------------------------------------------------------

// The context has no inputs any more: rala_hip_initialize, rala_hip_dedupe and the overlap columns are refused until a setter
// has succeeded.  ONLY that: the stage flags stay.  The sharded runner's ingest drops the slice context's inputs this way, and
// the results of the run before stay readable through rala_hip_mg_context when that ingest fails or finds an irregular file -
// as they always were.  The validity bits are not taken away either (rala_hip_get_valid keeps answering - with no overlaps
// it copies nothing): only new overlaps do that.
inline void inputs_dropped(rala_hip_ctx* ctx) {
    ctx->inputs_set = false;
    ctx->n_ovl = 0;
}

// A setter or a single-context ingest is about to write over the inputs: until it has succeeded (inputs_adopted) the context
// has none - no overlap columns either - and with them go the results: a call that fails half way leaves "reads set",
// whatever the state was.
inline void inputs_withdrawn(rala_hip_ctx* ctx) {
    inputs_dropped(ctx);
    ctx->ovl = OvlSoA();
    results_dropped(ctx);
}

// The caller's inputs of one kind are the context's (the setter began with inputs_withdrawn and has put its own pointers and
// counts in place): the other kinds' are cleared, the results dropped.  Bounds alone (tuples, records, blocks) initialize and answer per-read getters;
// rala_hip_construct needs overlaps.  New overlaps have no validity bits yet; bounds leave the bits of earlier overlaps
// readable (as inputs_dropped does).
inline void inputs_adopted(rala_hip_ctx* ctx, Inputs kind) {
    ctx->inputs_set = true;
    ctx->tuple_mode = kind != Inputs::kOverlaps;
    ctx->blocks_mode = kind == Inputs::kBlocks;
    ctx->dedupe_pending = false;
    if (kind == Inputs::kOverlaps) {
        ctx->valid_ready = false;
        ctx->n_tuples = 0;
    } else {
        ctx->upload_pending = false;
    }
    if (kind != Inputs::kTuples) ctx->tuples = nullptr;
    if (kind != Inputs::kRecords) { ctx->records = nullptr; ctx->n_records = 0; }
    if (kind != Inputs::kBlocks) { ctx->blocks_base = ctx->blocks_base_self = nullptr; ctx->n_block_records = 0; }
    results_dropped(ctx);
}

// RALA_HIP_MEM_HOST_ASYNC: the overlap columns are still the caller's host memory (rala_hip_initialize uploads them, any
// earlier reader through flush_upload) / they are on the device
inline void upload_deferred(rala_hip_ctx* ctx) { ctx->upload_pending = true; }
inline void upload_done(rala_hip_ctx* ctx) { ctx->upload_pending = false; }

// duplicate removal of a sharded run's sender runs on the side stream (event kEvEmitDedupeDone) / the second pass has joined it
inline void dedupe_forked(rala_hip_ctx* ctx) { ctx->dedupe_pending = true; }
inline void dedupe_joined(rala_hip_ctx* ctx) { ctx->dedupe_pending = false; }

// d_valid holds the validity bits of the context's overlaps: rala_hip_get_valid answers, a state may be installed beside them
inline void validity_bits_ready(rala_hip_ctx* ctx) { ctx->valid_ready = true; }

// ---- stages ----------------------------------------------------------------------------------------------------------

// rala_hip_initialize starts over: whatever it leaves behind when it fails is nobody's
inline void initialize_begun(rala_hip_ctx* ctx) {
    results_dropped(ctx);
    ctx->rowless = ctx->pile_rows == 0;
}

// Per-read state is on the device (rala_hip_initialize computed it, or it was installed from outside - after
// results_dropped): the per-read getters answer, rala_hip_construct may run.  rows_and_events: the pile rows (or, rowless,
// what they are rebuilt from) and the bound events are this context's too - without them the row getters and the sensitive
// pass are refused; events_in_fixed_slots: where those events lie.  A caller is told RALA_HIP_EFILTERED behind this
// transition: a context whose reads are all filtered IS initialized.
inline void state_installed(rala_hip_ctx* ctx, uint64_t n_prefiltered, uint32_t pool_used, bool rows_and_events,
                            bool events_in_fixed_slots, bool valid_ready) {
    ctx->n_prefiltered = n_prefiltered;
    ctx->pool_used = pool_used;
    ctx->piles_resident = ctx->ev_ready = rows_and_events;
    ctx->ev_fixed = rows_and_events && events_in_fixed_slots;
    ctx->valid_ready = valid_ready;
    ctx->initialized = true;
}

// rala_hip_construct has passed its checks: the last construct's repeat hills are gone
inline void construct_begun(rala_hip_ctx* ctx) { ctx->have_repeats = ctx->rep_host_stale = false; }
// ... and its second pass has succeeded: what an earlier, failed construct left on the device is nobody's (until here the
// getters still fetch it: a second pass that fails leaves the context as it found it)
inline void tail_begun(rala_hip_ctx* ctx) { ctx->tail_on_device = ctx->host_stale = false; }
// lists, graph and read state of the construct under way lie on the device; the host's copies come with the first getter
inline void tail_left_on_device(rala_hip_ctx* ctx) { ctx->tail_on_device = ctx->host_stale = true; }
// the graph is there: lists and graph answer, the transitive reduction may run, another construct is refused
inline void constructed(rala_hip_ctx* ctx) { ctx->constructed = true; }
// the sensitive pass behind a finished chimera stage failed: the context is initialized, not constructed
inline void construct_failed(rala_hip_ctx* ctx) { ctx->constructed = false; }

// ---- where the results lie -------------------------------------------------------------------------------------------

// the host's per-read vectors match the device (download_read_state)
inline void host_mirrors_fresh(rala_hip_ctx* ctx) { ctx->host_state_fresh = true; }
// ... and so do its lists and graph (materialize_host)
inline void host_lists_fetched(rala_hip_ctx* ctx) { ctx->host_stale = false; }

// the transitive marks of the device graph wait on the device for rala_hip_get_graph (ok: the stage succeeded) / were fetched
inline void marks_left_on_device(rala_hip_ctx* ctx, bool ok) { ctx->marks_on_device = ok; }
inline void marks_fetched(rala_hip_ctx* ctx) { ctx->marks_on_device = false; }

// the sensitive pass has left n hills on the device / the host's vectors hold them / they count: rala_hip_get_intervals(2)
// returns them, and (sensitive pass on cl's rows) cl's rows are rebuilt with the sensitive bounds on top
inline void repeat_hills_left_on_device(rala_hip_ctx* ctx, uint32_t n) { ctx->n_rep_hills = n; ctx->rep_host_stale = true; }
inline void repeat_hills_fetched(rala_hip_ctx* ctx) { ctx->rep_host_stale = false; }
inline void repeat_hills_found(rala_hip_ctx* ctx) { ctx->have_repeats = true; }
inline void sensitive_bounds_kept(rala_hip_ctx* cl) { cl->sens_csr_ready = true; }

}  // namespace rala_hip
