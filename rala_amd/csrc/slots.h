// The words of the small device buffers through which host and device hand counts and flags to each other, and the
// context's events, by name (DESIGN.md section 11 has the table).  One enumeration per owner of a buffer: the stages of a
// context follow each other on its main stream, so two owners of one word never overlap in time.  Words that are cleared
// or fetched in ONE copy are neighbours: the static_asserts say which.
#pragma once
#include <stdint.h>

namespace rala_hip {

// ---- d_small ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kSmallWords = 16;
// word 0 outlives the stages: the count of the primary interval pool, left by rala_hip_initialize or by an installed
// state (download_read_state fetches it with the first getter)
constexpr uint32_t kSmallPoolCount = 0;
// rala_hip_initialize: all sixteen cleared by its first fill, all sixteen fetched by its one look
enum InitSmall : uint32_t {
    kInitPoolCount = kSmallPoolCount,
    kInitStatus = 1,             // kErr* bits of the pile kernels
    kInitToCap2048 = 2,          // reads handed on by the cap-1024 kernels
    kInitDenseReads = 3,         // reads listed as event-dense
    kInitToCap1024 = 4,          // reads handed on by the cap-512 kernels
    kInitToPosition = 5,         // reads handed on to the position-space kernel
    kInitSlotOverflow = 6,       // a read with more events than a fixed slot holds
    kInitDeadReads = 7,
    kInitNotedReads = 8,         // reads noted for the lists in global memory
    kInitDedupeMarks = 9,        // marks of the counting pass's duplicate removal
};
// an installed state (finish_install, rala_hip_import_state): the pool's count and zeros behind it
constexpr uint32_t kInstallSmallWords = 8;
// the sensitive pass (preprocess_repeats, rala_hip_find_repetitive_hills): the pool's count and the status are cleared in one
// memset, the status and the noted reads fetched in one copy (run_repeats_kernel)
enum SensSmall : uint32_t {
    kSensBadRecord = 2,
    kSensPoolCount = 6,          // the repeat hills' pool
    kSensStatus = 7,             // kErr* bits of the repeat-hill kernels
    kSensNotedReads = 8,
};
constexpr uint32_t kSensPoolWords = 2, kSensLookWords = 2;
static_assert(kSensStatus == kSensPoolCount + 1, "pool count and status are cleared (and reset) together");
static_assert(kSensNotedReads == kSensStatus + 1, "status and noted reads are fetched together");
static_assert(kSensStatus + kSensLookWords <= kSmallWords && kSensPoolCount + kSensPoolWords <= kSmallWords, "inside d_small");
// the host's component loop (component_medians, use_gpu_tail = 0)
enum CcSmall : uint32_t { kCcChanged = 2 };
// the transitive reduction (tr_mark_device): both cleared by one fill, fetched in one copy
enum TrSmall : uint32_t { kTrBadEndpoint = 2, kTrPairs = 3 };
constexpr uint32_t kTrWords = 2;
static_assert(kTrPairs == kTrBadEndpoint + 1 && kTrBadEndpoint + kTrWords <= kSmallWords, "fetched together, inside d_small");
static_assert(kInitDedupeMarks < kSmallWords && kInstallSmallWords <= kSmallWords, "inside d_small");

// ---- d_counts --------------------------------------------------------------------------------------------------------
constexpr uint32_t kCountsWords = 48;
// pass 2: all of d_counts cleared by its first fill; the first eight words fetched by its one look
enum Pass2Counts : uint32_t {
    kPass2ReadsAlive = 0,
    kPass2Verdict = 1,           // launch_fixed_point_finish: the rounds did not settle
    kPass2FinishRounds = 2,      // ... and how many it took
    kPass2Survivors = 6,         // two words: overlaps, internals (launch_pair_offsets_pass)
    kPass2Sync = 32,             // launch_fixed_point_finish's sync8
};
constexpr uint32_t kPass2LookWords = 8, kPass2SyncWords = 8;
static_assert(kPass2Survivors + 2 <= kPass2LookWords, "the survivor counts come with the look");
static_assert(kPass2Sync + kPass2SyncWords <= kCountsWords, "inside d_counts");
// the tail (gpu_tail_part_a, gpu_tail_part_b): part b fetches the totals, the reads left and the containment scans' verdict
// in one copy
enum TailCounts : uint32_t {
    kTailDropped = 4,            // two words: overlaps dropped per round of a batch (part a)
    kTailTotals = 6,             // two words: kept items, dovetails (the last launch_segment_pass)
    kTailReadsLeft = 8,          // launch_node_pass
    kTailContain = 9,            // launch_tail_contain's 21 words, cleared (one more) by launch_tail_init; the first one: a scan failed
    kTailKillers = 10,           // four of them: the scans' killer counts (trace)
};
constexpr uint32_t kTailDroppedWords = 2, kTailLookWords = 4, kTailKillerWords = 4, kTailContainWords = 21, kTailInitWords = 22;
static_assert(kTailDropped + kTailDroppedWords <= kTailTotals, "the rounds' verdicts end in front of the totals");
static_assert(kTailReadsLeft == kTailTotals + 2 && kTailContain == kTailReadsLeft + 1 && kTailContain + 1 == kTailTotals + kTailLookWords,
              "totals, reads left and the scans' verdict are fetched together");
static_assert(kTailKillers > kTailContain && kTailKillers + kTailKillerWords <= kTailContain + kTailContainWords, "the killer counts are the scans'");
static_assert(kTailContain + kTailInitWords <= kPass2Sync && kTailContain + kTailContainWords <= kCountsWords, "inside d_counts, clear of sync8");

// ---- d_chain_cnt -----------------------------------------------------------------------------------------------------
constexpr uint32_t kChainWords = 16;
// the sensitive pass: the hand-over counts of a mode (run_sens_pass clears four words there, fetches the first two in one
// copy), the lengths of its two read lists (preprocess_repeats), the sizes of a mode's five classes (SensSplitArgs::counts)
enum ChainCnt : uint32_t {
    kChainFrom512 = 0,           // handed on by the cap-512 kernels
    kChainFrom1024 = 1,          // ... by the cap-1024 and cap-2048 kernels
    kChainTargets = 4,           // reads that received sensitive bounds (mode 1's list)
    kChainMembers = 5,           // reads with an overlap (mode 2's list)
    kChainClasses = 8,
};
constexpr uint32_t kChainHandedWords = 4, kChainLookWords = 2, kChainClassWords = 5;
static_assert(kChainFrom1024 == kChainFrom512 + 1 && kChainFrom512 + kChainLookWords <= kChainFrom512 + kChainHandedWords, "fetched together");
static_assert(kChainFrom512 + kChainHandedWords <= kChainTargets, "a mode's clear leaves the lists' lengths alone");
static_assert(kChainMembers < kChainClasses && kChainClasses + kChainClassWords <= kChainWords, "inside d_chain_cnt");
// the five classes of a mode, in the order of SensSplitArgs::out and ::counts
enum SensClass : uint32_t { kClassCap512 = 0, kClassCap512Long = 1, kClassCap1024 = 2, kClassCap2048 = 3, kClassPosition = 4 };
static_assert(kClassPosition + 1 == kChainClassWords, "one size per class");

// ---- d_cc_flags ------------------------------------------------------------------------------------------------------
constexpr uint32_t kCcFlagsWords = 8;
enum CcFlags : uint32_t {
    kCcInstallDead = 6,          // an installed state's filtered reads (finish_install)
    kCcTailChanged = 7,          // launch_cc_hook's "changed" in the tail's components (nobody reads it)
};
static_assert(kCcTailChanged < kCcFlagsWords, "inside d_cc_flags");

// ---- ctx->ev ---------------------------------------------------------------------------------------------------------
// An event with several roles has one name per role.  A hipStreamWaitEvent waits for the record that stands when it is
// enqueued, so a role is over once its last wait is enqueued and its times are read; the host enqueues a context's calls
// one after the other.  Beside each alias: why that has happened before the other role records.
enum Event : uint32_t {
    kEvInitBegin = 0,            // initialize's marks: its begin,
    kEvInitDedupeDone = 1,       // ... duplicate removal done (joined behind the pile kernels),
    kEvInitBucketed = 2,         // ... bounds bucketed (the aux stream and a late duplicate removal start behind it),
    kEvInitPilesDone = 3,        // ... pile kernels done
    kEvPass2Begin = 4, kEvPass2Classified = 5, kEvPass2Decided = 6, kEvPass2End = 7,      // pass 2's marks (pass2_times)
    kEvBucketCounted = 8,        // initialize: the bucketing's counting pass is done (the side stream waits)
    kEvAuxDrained = 9,           // initialize: what a failed call left on the aux stream has ended
    kEvTrBegin = 10, kEvTrEnd = 11,
    kEvCount = 12,
    // shard_emit's fork of its duplicate removal: initialize, a call of its own, has read kEvInitBegin's time before it returned
    kEvEmitCounted = kEvInitBegin,
    // shard_emit's duplicate removal done (pass 2 joins): both roles say the same of the same validity bits on the same
    // stream, so an initialize in between stands behind the emit's and pass 2 waits for both
    kEvEmitDedupeDone = kEvInitDedupeDone,
    // fork / join of a sharded run's survivor gather (pass 2; the join: gpu_tail_part_a): initialize has read its times
    // before any construct can run, and construct_stages calls pass 2 and part a one behind the other
    kEvGatherFork = kEvInitBucketed,
    kEvGatherJoin = kEvInitPilesDone,
    // initialize's aux pile kernels done: the side stream's wait for kEvBucketCounted is enqueued inside the bucketing, before
    kEvPileAuxDone = kEvBucketCounted,
    // a mode of the sensitive pass (run_sens_pass), inside construct and so behind an initialize that has returned: the
    // forked streams' waits are enqueued right behind the fork's record, the position stream's join far behind them
    kEvSensFork = kEvBucketCounted,
    kEvSensPosDone = kEvBucketCounted,
    // ... its aux stream's join: kEvAuxDrained's one wait is enqueued in the line behind its record, at the top of initialize
    kEvSensAuxDone = kEvAuxDrained,
};

}  // namespace rala_hip
