// C surface of rala::AssemblyGraph for the CPU test-suite (tests/test_layout_cpu.py): build a
// graph from arrays, run the clean-up stages, read the result back.  Not part of the product
// boundary (that is include/rala_hip.h + the rala:: classes).
#include <stdio.h>
#include <stdlib.h>
#include <sstream>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "assembly_graph.hpp"

namespace {

uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 1099511628211ull; }
    return h;
}

// the bytes of one node, whichever way the graph holds them (span mode: through the graph's speller; empty where it refuses)
std::string node_bytes(const rala::AssemblyGraph* g, uint64_t node) {
    if (!g->span_mode()) return g->nodes()[node].data;
    std::string bytes;
    std::vector<uint64_t> off;
    if (g->spell(std::vector<uint64_t>(1, node), bytes, off) != 0) bytes.clear();
    return bytes;
}

}  // namespace

extern "C" {

void* ag_create() { return new rala::AssemblyGraph(); }
void ag_destroy(void* h) { delete (rala::AssemblyGraph*)h; }

void ag_add_node_pair(void* h, uint64_t sequence_id, const char* name, const char* data, const char* rc) {
    ((rala::AssemblyGraph*)h)->add_sequence_nodes(sequence_id, name, data, rc);
}
// span mode (tests/test_spans_cpu.py): the pair as spans of source `source`; 0, or -1 where the graph holds strings
int ag_add_node_pair_spans(void* h, uint64_t sequence_id, const char* name, uint32_t source, uint32_t first, uint32_t len) {
    return ((rala::AssemblyGraph*)h)->add_sequence_node_spans(sequence_id, name, source, first, len) ? 0 : -1;
}
// the table of bases of a span-mode graph, copied: source s is bases[base_off[s] .. base_off[s + 1]); installs a plain host
// speller over it - the definition of a span, byte by byte, refusing what rala_hip_spell refuses
void ag_set_sources(void* h, const uint8_t* bases, const uint64_t* base_off, uint64_t n) {
    auto table = std::make_shared<std::pair<std::vector<uint8_t>, std::vector<uint64_t>>>();
    table->second.assign(base_off, base_off + n + 1);
    table->first.assign(bases, bases + base_off[n]);
    ((rala::AssemblyGraph*)h)->set_speller([table](const rala::AssemblyGraph::Span* spans, uint64_t n_spans, uint8_t* out, uint64_t out_bytes) {
        const std::vector<uint8_t>& B = table->first;
        const std::vector<uint64_t>& off = table->second;
        uint64_t at = 0;
        for (uint64_t k = 0; k < n_spans; ++k) {
            const auto& s = spans[k];
            if ((uint64_t)s.source + 1 >= off.size() || s.rc > 1) return -2;
            const uint64_t lo = off[s.source] + s.first, hi = lo + s.len;
            if (hi > off[s.source + 1] || at + s.len > out_bytes) return -2;
            for (uint64_t j = 0; j < s.len; ++j) {
                uint8_t c = s.rc ? B[hi - 1 - j] : B[lo + j];
                if (s.rc) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
                out[at + j] = c;
            }
            at += s.len;
        }
        return at == out_bytes ? 0 : -2;
    });
}
// a node's spans, four words each (source, first, len, rc): returns their number, copies at most cap of them
uint64_t ag_node_spans(void* h, uint64_t node, uint32_t* out, uint64_t cap) {
    const auto& sp = ((rala::AssemblyGraph*)h)->nodes()[node].spans;
    for (size_t k = 0; out && k < sp.size() && k < cap; ++k) {
        out[4 * k] = sp[k].source; out[4 * k + 1] = sp[k].first; out[4 * k + 2] = sp[k].len; out[4 * k + 3] = sp[k].rc;
    }
    return sp.size();
}
void ag_add_edge(void* h, uint32_t begin_node, uint32_t end_node, uint32_t length) {
    ((rala::AssemblyGraph*)h)->add_edge(begin_node, end_node, length);
}
void ag_mark_edge(void* h, uint32_t edge) { ((rala::AssemblyGraph*)h)->mark_edge(edge); }
void ag_note_transitive(void* h) { ((rala::AssemblyGraph*)h)->note_transitive_edges(); }
// engine: the layout steps (rala_hip_layout through a ctypes callback in the GPU tests)
typedef int (*ag_layout_fn)(uint32_t n, double* x, double* y, const uint32_t* adj_off, const uint32_t* adj,
                            uint32_t iterations, double k, double t, double dt);
int ag_postprocess(void* h, uint32_t seed, ag_layout_fn engine) {
    return ((rala::AssemblyGraph*)h)->postprocess(
        [engine](uint32_t n, double* x, double* y, const uint32_t* adj_off, const uint32_t* adj, uint32_t iterations,
                 double k, double t, double dt) { return engine(n, x, y, adj_off, adj, iterations, k, t, dt); },
        seed);
}
// engine: all components in one call (rala_hip_layout_batch through a ctypes callback in the GPU tests)
typedef int (*ag_layout_batch_fn)(uint32_t n_components, const uint32_t* comp_off, double* x, double* y,
                                  const uint32_t* adj_off, const uint32_t* adj, const double* k, uint32_t iterations,
                                  double t, double dt);
int ag_postprocess_batched(void* h, uint32_t seed, ag_layout_batch_fn engine) {
    return ((rala::AssemblyGraph*)h)->postprocess_batched(
        [engine](uint32_t n_components, const uint32_t* comp_off, double* x, double* y, const uint32_t* adj_off,
                 const uint32_t* adj, const double* k, uint32_t iterations, double t, double dt) {
            return engine(n_components, comp_off, x, y, adj_off, adj, k, iterations, t, dt);
        },
        seed);
}
void ag_edge_weights(void* h, double* w) {
    auto* g = (rala::AssemblyGraph*)h;
    for (size_t i = 0; i < g->edges().size(); ++i) w[i] = g->edges()[i].alive ? g->edges()[i].weight : 0.0;
}
uint64_t ag_transitive(void* h, uint64_t* pairs) {
    const auto& te = ((rala::AssemblyGraph*)h)->transitive_edges();
    if (pairs) for (size_t i = 0; i < te.size(); ++i) { pairs[2 * i] = te[i].first; pairs[2 * i + 1] = te[i].second; }
    return te.size();
}
void ag_remove_marked(void* h, int remove_nodes) { ((rala::AssemblyGraph*)h)->remove_marked_objects(remove_nodes != 0); }

// op: 0 remove_tips, 1 remove_bubbles, 2 create_unitigs, 3 shrink(arg), 4 remove_long_edges
uint32_t ag_run(void* h, int op, uint32_t arg) {
    auto* g = (rala::AssemblyGraph*)h;
    switch (op) {
        case 0: return g->remove_tips();
        case 1: return g->remove_bubbles();
        case 2: return g->create_unitigs();
        case 3: return g->shrink(arg);
        case 4: return g->remove_long_edges();
    }
    return 0xFFFFFFFFu;
}

void ag_size(void* h, uint64_t* n_nodes, uint64_t* n_edges) {
    auto* g = (rala::AssemblyGraph*)h;
    *n_nodes = g->nodes().size();
    *n_edges = g->edges().size();
}

// per node: alive, length, number of reads, hash of the sequence, hash of the read ids,
// first / last orientation, in / out degree, hash of the adjacency lists (edge ids in order)
void ag_dump_nodes(void* h, uint8_t* alive, uint32_t* length, uint32_t* n_seq, uint64_t* data_hash, uint64_t* ids_hash,
                   uint8_t* first_rc, uint8_t* last_rc, uint32_t* indeg, uint32_t* outdeg, uint64_t* adj_hash) {
    auto* g = (rala::AssemblyGraph*)h;
    // span mode: every live node's bytes with one call of the speller
    std::string bytes;
    std::vector<uint64_t> ids, off;
    std::vector<int64_t> at(g->nodes().size(), -1);
    if (g->span_mode()) {
        for (size_t i = 0; i < g->nodes().size(); ++i) {
            if (!g->nodes()[i].alive) continue;
            at[i] = (int64_t)ids.size();
            ids.push_back(i);
        }
        if (g->spell(ids, bytes, off) != 0) bytes.assign(bytes.size(), '?');
    }
    for (size_t i = 0; i < g->nodes().size(); ++i) {
        const auto& n = g->nodes()[i];
        alive[i] = n.alive;
        length[i] = n.length();
        n_seq[i] = (uint32_t)n.sequence_ids.size();
        data_hash[i] = at[i] >= 0 ? fnv1a(bytes.data() + off[at[i]], off[at[i] + 1] - off[at[i]]) : fnv1a(n.data.data(), n.data.size());
        ids_hash[i] = fnv1a(n.sequence_ids.data(), n.sequence_ids.size() * 8);
        first_rc[i] = n.is_first_rc; last_rc[i] = n.is_last_rc;
        indeg[i] = n.indegree(); outdeg[i] = n.outdegree();
        uint64_t a = fnv1a(n.prefix_edges.data(), n.prefix_edges.size() * 4);
        adj_hash[i] = fnv1a(n.suffix_edges.data(), n.suffix_edges.size() * 4, a);
        if (!n.alive) first_rc[i] = last_rc[i] = 0;
    }
}

void ag_dump_edges(void* h, uint8_t* alive, uint32_t* begin_node, uint32_t* end_node, uint32_t* length) {
    auto* g = (rala::AssemblyGraph*)h;
    for (size_t i = 0; i < g->edges().size(); ++i) {
        const auto& e = g->edges()[i];
        alive[i] = e.alive;
        begin_node[i] = e.alive ? e.begin_node : 0; end_node[i] = e.alive ? e.end_node : 0;
        length[i] = e.alive ? e.length : 0;
    }
}

// kind 0 csv, 1 gfa, 2 json (piles as "<id>":{} stand-ins); returns the length, copies at most cap bytes
uint64_t ag_print(void* h, int kind, char* dst, uint64_t cap) {
    const rala::AssemblyGraph* g = (const rala::AssemblyGraph*)h;
    std::string s;
    if (kind == 2) {
        std::ostringstream os;
        g->write_json(os, [](uint64_t id) { return "\"" + std::to_string(id) + "\":{}"; });
        s = os.str();
    } else {
        char* buf = nullptr;
        size_t len = 0;
        FILE* f = open_memstream(&buf, &len);
        if (kind == 0) g->write_csv(f); else g->write_gfa(f);
        fclose(f);
        s.assign(buf, len);
        free(buf);
    }
    if (dst) memcpy(dst, s.data(), s.size() < cap ? s.size() : cap);
    return s.size();
}

uint64_t ag_node_data(void* h, uint64_t node, char* dst, uint64_t cap) {
    const std::string d = node_bytes((rala::AssemblyGraph*)h, node);
    if (dst && cap >= d.size()) memcpy(dst, d.data(), d.size());
    return d.size();
}

}  // extern "C"
