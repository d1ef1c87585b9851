"""Node bases as spans: the definition of a span as a Python speller, and the product's assembly graph in span mode
(rala_amd/host/libassembly_graph.so: ag_add_node_pair_spans, ag_set_sources, ag_node_spans) beside the drivers of layout.py."""
import ctypes
import os

import numpy as np

import layout

COMP = np.arange(256, dtype=np.uint8)
for _a, _b in (b"AT", b"TA", b"CG", b"GC"):
    COMP[_a] = _b


def spell(bases, base_off, spans):
    """what spans (rows of source, first, len, rc) of the table spell: source s is bases[base_off[s]:base_off[s + 1]];
    rc = 0: out[j] = B[first + j]; rc = 1: out[j] = comp(B[first + len - 1 - j]), comp A <-> T, C <-> G in upper case only"""
    out = [np.zeros(0, dtype=np.uint8)]
    for s, first, n, rc in np.asarray(spans, dtype=np.int64).reshape(-1, 4):
        B = bases[int(base_off[s]):int(base_off[s + 1])]
        assert rc in (0, 1) and first + n <= len(B)
        piece = B[first:first + n]
        out.append(COMP[piece[::-1]] if rc else piece)
    return np.concatenate(out)


def pack(sources):
    """list of bytes -> (bases, base_off) of a table"""
    base_off = np.zeros(len(sources) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in sources], out=base_off[1:])
    return np.frombuffer(b"".join(sources), dtype=np.uint8), base_off


class SpanGraph(layout._Graph):
    """the product graph in span mode: nodes are added as (source, first, len), sources() installs the table and the host
    speller; everything else is layout._Graph (node_data and dump's data_hash go through the speller)"""

    def __init__(self):
        super().__init__(ctypes.CDLL(os.path.join(layout.ROOT, "rala_amd", "host", "libassembly_graph.so")), "ag_")
        f = self.f
        f("add_node_pair_spans").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        f("add_node_pair_spans").restype = ctypes.c_int
        f("set_sources").argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        f("set_sources").restype = None
        f("node_spans").argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
        f("node_spans").restype = ctypes.c_uint64
        self.table = None

    def add_node_pair_spans(self, seq_id, name, source, first, length):
        return int(self.f("add_node_pair_spans")(self.h, seq_id, name, source, first, length))

    def set_sources(self, sources):
        self.table = pack(sources)
        bases, base_off = self.table
        self.f("set_sources")(self.h, bases.ctypes.data if len(bases) else None, base_off.ctypes.data, len(sources))

    def node_spans(self, node):
        n = int(self.f("node_spans")(self.h, node, None, 0))
        out = np.zeros((n, 4), dtype=np.uint32)
        if n:
            self.f("node_spans")(self.h, node, out.ctypes.data, n)
        return out

    def n_nodes(self):
        nn, ne = ctypes.c_uint64(), ctypes.c_uint64()
        self.f("size")(self.h, ctypes.byref(nn), ctypes.byref(ne))
        return nn.value


def assert_same_bases(span_graph, strings, what="", forward_only=False):
    """every live node: the length, and what its spans spell - by the product's speller (node_data) AND by the Python one -
    against the bytes the graph of strings holds"""
    (na, _), (nb, _) = span_graph.dump(), strings.dump()
    assert (na["alive"] == nb["alive"]).all(), "%s: live nodes differ" % what
    bases, base_off = span_graph.table
    for k in np.nonzero(na["alive"])[0]:
        if forward_only and k % 2:
            continue
        want = strings.node_data(int(k))
        assert int(na["length"][k]) == len(want), "%s node %d: length %d, the strings' %d" % (what, k, na["length"][k], len(want))
        sp = span_graph.node_spans(int(k))
        assert int(sp[:, 2].astype(np.int64).sum()) == len(want), "%s node %d: the spans' lengths" % (what, k)
        assert spell(bases, base_off, sp).tobytes() == want, "%s node %d: the spans spell other bytes" % (what, k)
        assert span_graph.node_data(int(k)) == want, "%s node %d: the product's speller" % (what, k)
