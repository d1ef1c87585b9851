// librala_hip: the cross-check path of rala_hip_construct (option use_gpu_tail = 0) - the short sequential tail of
// Graph::preprocess on the host, over the few per cent of overlaps that survive containment removal (connected components,
// component medians, iterate-until-stable), and the graph built from what is left.  Implements no call of rala_hip.h by
// itself: construct.hip and sensitive.hip call it (orchestration.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orchestration.h"

using namespace rala_hip;

uint32_t rala_hip::host_type(rala_hip_ctx* ctx, const HostOvl& o) {
    return ovl_type(o.c, o.strand, ctx->h_begin[o.a], ctx->h_end[o.a], ctx->h_begin[o.b], ctx->h_end[o.b]);
}

namespace {

// ---- host tail helpers (Graph::preprocess, graph.cpp:699-880) --------------------------
bool host_trim(rala_hip_ctx* ctx, HostOvl& o) {
    if (!ctx->h_alive[o.a] || !ctx->h_alive[o.b]) return false;
    return ovl_trim(o.c, o.strand, ctx->h_begin[o.a], ctx->h_end[o.a], ctx->h_begin[o.b], ctx->h_end[o.b]);
}

// Overlap::trim is idempotent while both valid regions stand still, so only overlaps that
// touch a read whose region changed since the last pass ("dirty") are recomputed.  Dropped
// items stay in place with dead = 1 (lists are compacted once, at the end); the pass is
// data parallel over the host pool.  Returns the number of items dropped.
uint64_t retrim(rala_hip_ctx* ctx, std::vector<HostOvl>& v) {
    const uint8_t* dirty = ctx->dirty.data();
    std::vector<uint64_t> dropped(ctx->pool->size(), 0);
    ctx->pool->chunks(v.size(), [&](unsigned t, size_t b, size_t e) {
        uint64_t d = 0;
        for (size_t k = b; k < e; ++k) {
            HostOvl& o = v[k];
            if (o.dead || !(dirty[o.a] | dirty[o.b])) continue;
            if (!host_trim(ctx, o)) { o.dead = 1; ++d; }
            else o.type = 255;
        }
        dropped[t] = d;
    });
    uint64_t total = 0;
    for (uint64_t d : dropped) total += d;
    return total;
}

// flags only (callable from pool threads, one read per thread); collect_dirty() lists them
void mark_dirty(rala_hip_ctx* ctx, uint32_t r) {
    ctx->dirty[r] = 1;
    ctx->ever_dirty[r] = 1;
}

void collect_dirty(rala_hip_ctx* ctx, const std::vector<uint32_t>& among) {
    for (uint32_t r : among) if (ctx->dirty[r]) ctx->dirty_list.push_back(r);
}

void clear_dirty(rala_hip_ctx* ctx) {
    for (uint32_t r : ctx->dirty_list) ctx->dirty[r] = 0;
    ctx->dirty_list.clear();
}

bool host_shrink(rala_hip_ctx* ctx, uint32_t r, uint32_t b, uint32_t e) {
    if (b > e || e - b < kMinRegion) { mark_dirty(ctx, r); return false; }
    if (ctx->h_begin[r] != b || ctx->h_end[r] != e) mark_dirty(ctx, r);
    ctx->h_begin[r] = b;
    ctx->h_end[r] = e;
    return true;
}

// Pile::break_over_chimeric_hills (pile.cpp:471-498): geom.h longest_piece, as on the device
bool break_hills(rala_hip_ctx* ctx, uint32_t r, const Interval* hills, uint32_t n) {
    const Piece keep = longest_piece(ctx->h_begin[r], ctx->h_end[r], n,
                                     [&](uint32_t i, uint32_t& f, uint32_t& s) { f = hills[i].first; s = hills[i].second; },
                                     [&](uint32_t i) { return hills[i].aux <= 3; });
    return host_shrink(ctx, r, keep.begin, keep.end);
}

// Pile::break_over_chimeric_pits (pile.cpp:366-402); a pit is real when some
// coverage inside it satisfies data*1.84 <= median — monotone in data, so the
// minimum recorded by the pile kernel decides.  Unreal pits are kept (in place).
bool break_pits(rala_hip_ctx* ctx, uint32_t r, Interval* pits, uint32_t& n_pits, uint16_t dataset_median) {
    uint32_t w = 0;
    const Piece keep = longest_piece(ctx->h_begin[r], ctx->h_end[r], n_pits,
                                     [&](uint32_t k, uint32_t& f, uint32_t& s) { f = pits[k].first; s = pits[k].second; },
                                     [&](uint32_t k) {
                                         if ((double)pits[k].aux * 1.84 <= (double)dataset_median) return true;
                                         pits[w++] = pits[k];
                                         return false;
                                     });
    n_pits = w;
    return host_shrink(ctx, r, keep.begin, keep.end);
}

}  // namespace

// per read: the median of the pile medians of its connected component over the current
// overlaps (graph.cpp:740-783); components by min-label hooking on the GPU (cc_kernels).
int rala_hip::component_medians(rala_hip_ctx* ctx, std::vector<uint32_t>& members, std::vector<uint16_t>& med_of_member) {
    const size_t m = ctx->overlaps.size();
    members.clear();
    med_of_member.clear();
    if (m == 0) return RALA_HIP_OK;
    hipStream_t s = ctx->stream;
    // work on the ranks of the reads that were alive after the second pass (about a tenth of all)
    const std::vector<uint32_t>& rank = ctx->alive_rank;
    const std::vector<uint32_t>& reads = ctx->alive_reads;
    const size_t na = reads.size();
    HIPCHECK(ctx->p_cc_edges.ensure(2 * m));
    HIPCHECK(ctx->p_cc_label.ensure(na));
    uint32_t* edges = ctx->p_cc_edges.p;
    std::vector<uint8_t>& touched = ctx->scratch_touched;
    touched.assign(na, 0);
    ctx->pool->chunks(m, [&](unsigned, size_t b0, size_t e0) {
        for (size_t k = b0; k < e0; ++k) {
            const HostOvl& o = ctx->overlaps[k];
            if (o.dead) { edges[2 * k] = 0; edges[2 * k + 1] = 0; continue; }      // harmless self loop
            const uint32_t ra = rank[o.a], rb = rank[o.b];
            edges[2 * k] = ra; edges[2 * k + 1] = rb;
            touched[ra] = 1; touched[rb] = 1;
        }
    });
    HIPCHECK(ctx->d_cc_edges.ensure(2 * m));
    HIPCHECK(ctx->d_cc_label.ensure(na));
    HIPCHECK(hipMemcpyAsync(ctx->d_cc_edges.p, edges, 2 * m * 4, hipMemcpyHostToDevice, s));
    launch_cc_init(ctx->d_cc_label.p, (uint32_t)na, s);
    for (int round = 0;; ++round) {
        HIPCHECK(hipMemsetAsync(ctx->d_small.p + kCcChanged, 0, 4, s));
        for (int it = 0; it < 4; ++it) {          // several hook + jump steps per host round trip
            launch_cc_hook(ctx->d_cc_edges.p, (uint32_t)m, 0, ctx->d_cc_label.p, ctx->d_small.p + kCcChanged, s);
            launch_cc_compress(ctx->d_cc_label.p, (uint32_t)na, s);
        }
        uint32_t changed = 0;
        HIPCHECK(d2h_small(ctx, &changed, ctx->d_small.p + kCcChanged, 4, s));
        HIPCHECK(stream_sync(ctx, s));
        if (!changed) break;
        if (round > 10000) return fail(ctx, RALA_HIP_EDEVICE, "connected components did not converge");
    }
    uint32_t* label = ctx->p_cc_label.p;
    HIPCHECK(hipMemcpyAsync(label, ctx->d_cc_label.p, na * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(stream_sync(ctx, s));
    // members = reads with at least one overlap, in read order; grouped by label (counting sort)
    std::vector<uint32_t>& mrank = ctx->scratch_u32a;
    mrank.clear();
    for (size_t q = 0; q < na; ++q) if (touched[q]) { members.push_back(reads[q]); mrank.push_back((uint32_t)q); }
    std::vector<uint32_t>& cnt = ctx->scratch_u32b;
    cnt.assign(na + 1, 0);
    for (uint32_t q : mrank) ++cnt[label[q] + 1];
    for (size_t q = 0; q < na; ++q) cnt[q + 1] += cnt[q];
    std::vector<uint32_t> idx(members.size());
    for (size_t k = 0; k < members.size(); ++k) idx[cnt[label[mrank[k]]]++] = (uint32_t)k;
    med_of_member.assign(members.size(), 0);
    std::vector<uint16_t> mm;
    for (size_t b0 = 0; b0 < idx.size();) {
        const uint32_t lab = label[mrank[idx[b0]]];
        size_t t = b0;
        mm.clear();
        while (t < idx.size() && label[mrank[idx[t]]] == lab) { mm.push_back(ctx->h_median[members[idx[t]]]); ++t; }
        std::nth_element(mm.begin(), mm.begin() + mm.size() / 2, mm.end());
        const uint16_t med = mm[mm.size() / 2];
        for (size_t k = b0; k < t; ++k) med_of_member[idx[k]] = med;
        b0 = t;
    }
    return RALA_HIP_OK;
}

int rala_hip::preprocess_chimeras(rala_hip_ctx* ctx) {
    Trace tr;
    const uint64_t n = ctx->n_reads;
    ctx->dirty.assign(n, 0);
    ctx->ever_dirty.assign(n, 0);
    ctx->dirty_list.clear();
    ctx->alive_rank.assign(n, 0xFFFFFFFFu);
    ctx->alive_reads.clear();
    for (uint64_t r = 0; r < n; ++r) {
        if (!ctx->h_alive[r]) continue;
        ctx->alive_rank[r] = (uint32_t)ctx->alive_reads.size();
        ctx->alive_reads.push_back((uint32_t)r);
    }
    const std::vector<uint32_t>& n_pits0 = ctx->h_n_pits0;     // hills sit behind the initial pits
    ctx->h_n_pits0 = ctx->h_n_pits;
    // break over chimeric hills (graph.cpp:704-720)
    for (uint32_t r : ctx->alive_reads) {
        if (ctx->h_n_hills[r] == 0) continue;
        const Interval* hills = ctx->h_pool.data() + ctx->h_slot[r] + n_pits0[r];
        if (!break_hills(ctx, (uint32_t)r, hills, ctx->h_n_hills[r])) ctx->h_alive[r] = 0;
        ctx->h_n_hills[r] = 0;
    }
    collect_dirty(ctx, ctx->alive_reads);
    tr("break hills", ctx->dirty_list.size());
    retrim(ctx, ctx->overlaps);      // :722-728
    retrim(ctx, ctx->internals);     // :730-736
    clear_dirty(ctx);
    tr("retrim ov+int", ctx->overlaps.size() + ctx->internals.size());

    std::vector<uint32_t> members;
    std::vector<uint16_t> med;
    for (;;) {                       // :738-829
        const int rc = component_medians(ctx, members, med);
        if (rc != RALA_HIP_OK) return rc;
        tr("component medians", members.size());
        ctx->pool->chunks(members.size(), [&](unsigned, size_t b0, size_t e0) {
            for (size_t k = b0; k < e0; ++k) {
                const uint32_t r = members[k];
                if (ctx->h_n_pits[r] == 0) continue;     // no pits: shrink(begin, end) is a no-op
                Interval* pits = ctx->h_pool.data() + ctx->h_slot[r];
                if (!break_pits(ctx, r, pits, ctx->h_n_pits[r], med[k])) ctx->h_alive[r] = 0;
            }
        });
        collect_dirty(ctx, members);
        const bool changed = retrim(ctx, ctx->overlaps) != 0;
        // internals whose reads moved: trim again; the ones that became dovetails join the
        // overlaps, in internals order (graph.cpp:809-824)
        {
            const uint8_t* dirty = ctx->dirty.data();
            std::vector<HostOvl>& in = ctx->internals;
            std::vector<std::vector<uint32_t>> promoted(ctx->pool->size());
            ctx->pool->chunks(in.size(), [&](unsigned t, size_t b, size_t e) {
                for (size_t k = b; k < e; ++k) {
                    HostOvl& o = in[k];
                    // untouched since it was classified: still trimmed and still kX
                    if (o.dead || !((dirty[o.a] | dirty[o.b]) || o.type == 255)) continue;
                    if (!host_trim(ctx, o)) { o.dead = 1; continue; }
                    o.type = (uint8_t)host_type(ctx, o);
                    if (o.type == kTypeAB || o.type == kTypeBA) promoted[t].push_back((uint32_t)k);
                }
            });
            for (const auto& list : promoted) {
                for (uint32_t k : list) {
                    ctx->overlaps.push_back(in[k]);
                    in[k].dead = 1;
                }
            }
        }
        tr("break pits + retrim", ctx->dirty_list.size());
        clear_dirty(ctx);
        if (!changed) break;
    }

    // in-order containment removal without the chimera guard (:831-877); stale types are
    // refreshed in parallel first, the scan itself is sequential and cheap
    auto refresh = [&](std::vector<HostOvl>& v) {
        ctx->pool->chunks(v.size(), [&](unsigned, size_t b, size_t e) {
            for (size_t k = b; k < e; ++k) {
                HostOvl& o = v[k];
                if (!o.dead && o.type == 255 && ctx->h_alive[o.a] && ctx->h_alive[o.b]) o.type = (uint8_t)host_type(ctx, o);
            }
        });
    };
    // only containment overlaps (kA / kB) can delete a read: collect them in order (parallel),
    // walk them sequentially, then drop the items that had lost a read by the time the
    // reference's loop reached them (parallel; kill_pos = position of the deleting item)
    std::vector<uint32_t> kill_pos;
    auto kill_scan = [&](std::vector<HostOvl>& v, bool timed) {
        std::vector<std::vector<uint32_t>> cand(ctx->pool->size());
        ctx->pool->chunks(v.size(), [&](unsigned t, size_t b0, size_t e0) {
            for (size_t k = b0; k < e0; ++k) {
                const HostOvl& o = v[k];
                if (!o.dead && (o.type == kTypeA || o.type == kTypeB)) cand[t].push_back((uint32_t)k);
            }
        });
        if (timed) kill_pos.assign(n, 0xFFFFFFFFu);
        for (const auto& list : cand) {
            for (uint32_t k : list) {
                HostOvl& o = v[k];
                o.dead = 1;
                if (!ctx->h_alive[o.a] || !ctx->h_alive[o.b]) continue;
                const uint32_t victim = o.type == kTypeA ? o.b : o.a;
                ctx->h_alive[victim] = 0;
                if (timed) kill_pos[victim] = k;
            }
        }
        if (!timed) return;       // overlaps: a final sweep drops everything that lost a read
        ctx->pool->chunks(v.size(), [&](unsigned, size_t b0, size_t e0) {
            for (size_t k = b0; k < e0; ++k) {
                HostOvl& o = v[k];
                if (o.dead) continue;
                const bool gone_a = !ctx->h_alive[o.a] && (kill_pos[o.a] == 0xFFFFFFFFu || kill_pos[o.a] < k);
                const bool gone_b = !ctx->h_alive[o.b] && (kill_pos[o.b] == 0xFFFFFFFFu || kill_pos[o.b] < k);
                if (gone_a || gone_b) o.dead = 1;
            }
        });
    };
    refresh(ctx->overlaps);
    refresh(ctx->internals);
    kill_scan(ctx->overlaps, false);
    kill_scan(ctx->internals, true);
    tr("kill scans");
    // one compaction at the end: what is dead or (overlaps only, :869-877) lost a read goes
    auto compact = [&](std::vector<HostOvl>& v, bool check_piles) {
        const unsigned T = ctx->pool->size();
        std::vector<size_t> kept_to(T + 1, 0);
        auto keep = [&](const HostOvl& o) {
            return !o.dead && !(check_piles && (!ctx->h_alive[o.a] || !ctx->h_alive[o.b]));
        };
        const bool single = v.size() < 4096;
        ctx->pool->chunks(v.size(), [&](unsigned t, size_t b0, size_t e0) {
            size_t c = 0;
            for (size_t k = b0; k < e0; ++k) c += keep(v[k]);
            kept_to[t + 1] = c;
        });
        for (unsigned t = 0; t < T; ++t) kept_to[t + 1] += kept_to[t];
        std::vector<HostOvl>& out = ctx->scratch_ovl;      // capacity survives across calls
        out.resize(single ? kept_to[1] : kept_to[T]);
        ctx->pool->chunks(v.size(), [&](unsigned t, size_t b0, size_t e0) {
            size_t w = single ? 0 : kept_to[t];
            for (size_t k = b0; k < e0; ++k) if (keep(v[k])) out[w++] = v[k];
        });
        v.swap(out);
    };
    compact(ctx->internals, false);
    compact(ctx->overlaps, true);
    tr("compact", ctx->overlaps.size());
    return RALA_HIP_OK;
}

// nodes for the surviving reads, two edges per dovetail overlap (graph.cpp:553-632)
void rala_hip::build_graph(rala_hip_ctx* ctx) {
    const uint64_t n = ctx->n_reads;
    std::vector<uint32_t> read_to_node(n, 0xFFFFFFFFu);
    ctx->node_read.clear();
    for (uint64_t r = 0; r < n; ++r) {
        if (!ctx->h_alive[r]) continue;
        read_to_node[r] = (uint32_t)ctx->node_read.size();
        ctx->node_read.push_back((uint32_t)r);
        ctx->node_read.push_back((uint32_t)r);
    }
    const std::vector<HostOvl>& ov = ctx->overlaps;
    const size_t m = ov.size();
    std::vector<EdgePair>& ep = ctx->scratch_ep;
    std::vector<uint8_t>& has = ctx->scratch_has;
    ep.resize(m);
    has.assign(m, 0);
    const unsigned T = ctx->pool->size();
    std::vector<uint64_t> cnt(T + 1, 0);
    ctx->pool->chunks(m, [&](unsigned t, size_t b, size_t e) {
        uint64_t c = 0;
        for (size_t k = b; k < e; ++k) {
            const HostOvl& o = ov[k];
            const uint32_t Ba = ctx->h_begin[o.a], Ea = ctx->h_end[o.a], Bb = ctx->h_begin[o.b], Eb = ctx->h_end[o.b];
            const uint32_t ty = ovl_type(o.c, o.strand, Ba, Ea, Bb, Eb);
            if (ovl_edges(o.c, o.strand, ty, read_to_node[o.a], read_to_node[o.b], Ba, Ea, Bb, Eb, ep[k])) {
                has[k] = 1;
                ++c;
            }
        }
        cnt[t + 1] = c;
    });
    for (unsigned t = 0; t < T; ++t) cnt[t + 1] += cnt[t];
    const uint64_t ne = 2 * cnt[T];
    ctx->e_src.resize(ne); ctx->e_dst.resize(ne); ctx->e_len.resize(ne);
    ctx->pool->chunks(m, [&](unsigned t, size_t b, size_t e) {
        uint64_t w = 2 * (m < 4096 ? 0 : cnt[t]);
        for (size_t k = b; k < e; ++k) {
            if (!has[k]) continue;
            const EdgePair& p = ep[k];
            ctx->e_src[w] = p.src0; ctx->e_dst[w] = p.dst0; ctx->e_len[w] = p.len0;
            ctx->e_src[w + 1] = p.src1; ctx->e_dst[w + 1] = p.dst1; ctx->e_len[w + 1] = p.len1;
            w += 2;
        }
    });
    ctx->e_mark.assign(ne, 0);
}
