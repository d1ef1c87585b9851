"""GPU: the context's table of bases and rala_hip_spell (rala_amd/csrc/spell.hip, spell_kernels.hip) against the Python
speller of spans.py: every alignment of source and output, both strands, spans shorter than a word and longer than a tile,
more spans in a tile than LDS stages, windows whose edges fall inside spans; the refusals; the table's life; and the table
that rala_hip_slice_sequences leaves with the option keep_bases."""
import ctypes
import gzip

import numpy as np
import pytest

from rala_amd import hip
from rala_amd.synth import Dataset

import spans
import test_sequences_cpu as host

pytestmark = pytest.mark.gpu

TILE = 16384
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 16383, 16384, 16385, 40000]
BIG = len(LENGTHS) - 1
EINVAL = -2


def _table():
    rng = np.random.default_rng(11)
    sources = []
    for n in LENGTHS:
        b = rng.choice(np.frombuffer(b"ACGTACGTACGTNacgtn", dtype=np.uint8), size=n)
        if n == 40000:
            b[1000:1256] = np.arange(256, dtype=np.uint8)        # every byte value: most of them the complement leaves alone
            b[2000:2256] = np.arange(256, dtype=np.uint8)[::-1]
        sources.append(b.tobytes())
    return spans.pack(sources)


def _lists(base_off):
    """name -> (n, 4) array of spans"""
    L = {}
    # every (source address mod 16, output offset mod 16), forward and reverse: 100 bytes; a span of 1 .. 15 bytes in front
    # moves the output to where it has to be
    rows, pos, at = [], 0, 0
    for rc in (0, 1):
        for sa in range(16):
            for oa in range(16):
                fill = (oa - pos) % 16
                if fill:
                    rows.append((4, 3, fill, (sa + oa) & 1))
                    pos += fill
                first = 300 + 61 * at
                first += (sa - (int(base_off[BIG]) + first)) % 16
                assert (int(base_off[BIG]) + first) % 16 == sa and pos % 16 == oa
                rows.append((BIG, first, 100, rc))
                pos += 100
                at += 1
    L["alignments"] = rows
    L["short"] = [(s, f, n, rc) for rc in (0, 1) for n in (0, 1, 63, 64, 65) for s, f in ((6, 0), (BIG, 999), (8, 16384 - 65))]
    L["three_tiles"] = [(3, 0, 5, 1), (BIG, 0, 40000, 0), (2, 1, 7, 0), (BIG, 0, 40000, 1)]
    L["one_byte_spans"] = [(BIG, (k * 7) % 40000, 1, k & 1) for k in range(5000)]
    L["same_source"] = [(4, k % 40, 63 - k % 40, k % 3 == 0) for k in range(200)] + [(8, 0, 16384, k & 1) for k in range(3)]
    L["total_0"] = []
    L["total_0_of_empty_spans"] = [(0, 0, 0, 0), (5, 64, 0, 1), (BIG, 40000, 0, 0)]
    L["total_1"] = [(0, 0, 1, 1)]
    L["total_16384"] = [(7, 0, 16383, 1), (0, 0, 1, 0)]
    L["total_16385"] = [(9, 0, 16385, 1)]
    L["empty_spans_at_edges"] = [(1, 2, 0, 0), (8, 0, 16384, 0), (1, 15, 0, 1), (2, 0, 0, 0), (BIG, 1000, 300, 1), (3, 17, 0, 0)]
    return {k: np.array(v, dtype=np.uint32).reshape(-1, 4) for k, v in L.items()}


@pytest.fixture(scope="module")
def case():
    """the table, the span lists and what they spell (computed once), on one context"""
    bases, base_off = _table()
    assert len(np.unique(bases)) == 256
    lists = _lists(base_off)
    want = {k: spans.spell(bases, base_off, v) for k, v in lists.items()}
    ctx = hip.Context(0)
    ctx.set_bases(bases, base_off)
    yield {"ctx": ctx, "bases": bases, "base_off": base_off, "lists": lists, "want": want}
    ctx.close()


NAMES = ["alignments", "short", "three_tiles", "one_byte_spans", "same_source", "total_0", "total_0_of_empty_spans", "total_1",
         "total_16384", "total_16385", "empty_spans_at_edges"]


@pytest.mark.parametrize("window", [0, 16384, 32768])
@pytest.mark.parametrize("name", NAMES)
def test_spans_spell_what_python_spells(case, name, window):
    ctx, sp, want = case["ctx"], case["lists"][name], case["want"][name]
    ctx.set_option("debug_spell_window", window)
    try:
        got = ctx.spell(sp)
    finally:
        ctx.set_option("debug_spell_window", 0)
    assert len(got) == len(want)
    if not (got == want).all():
        i = int(np.nonzero(got != want)[0][0])
        raise AssertionError("%s, window %d: byte %d of %d is %d, not %d" % (name, window, i, len(want), got[i], want[i]))
    info = ctx.spell_info()
    w = window or 256 << 20
    assert info["spans"] == len(sp) and info["bytes"] == len(want)
    assert info["windows"] == info["launches"] == (len(want) + w - 1) // w
    assert info["sources"] == len(LENGTHS) and info["source_bytes"] == sum(LENGTHS) and info["from_slice"] == 0


def test_lists_cover_what_they_are_meant_to(case):
    L, want = case["lists"], case["want"]
    assert len(want["three_tiles"]) > 2 * TILE and len(want["one_byte_spans"]) == 5000 > 256
    assert len(want["alignments"]) > 3 * TILE                   # window edges inside spans of either strand
    assert [len(want["total_%s" % k]) for k in ("0", "1", "16384", "16385")] == [0, 1, 16384, 16385]
    off = np.concatenate([[0], np.cumsum(L["empty_spans_at_edges"][:, 2])])
    assert off[2] == TILE and L["empty_spans_at_edges"][2, 2] == 0 and L["empty_spans_at_edges"][3, 2] == 0
    # the complement leaves 252 of the 256 byte values alone, and the reverse spans meet all of them
    rc = want["three_tiles"][-40000:]
    assert len(np.unique(rc)) == 256


def _raw_spell(ctx, sp, out, out_bytes):
    sp = np.ascontiguousarray(sp, dtype=np.uint32).reshape(-1, 4)
    return ctx.L.rala_hip_spell(ctx.h, sp.ctypes.data, len(sp), out.ctypes.data, int(out_bytes))


def test_refusals_touch_nothing(case):
    bases, base_off = case["bases"], case["base_off"]
    good, want = case["lists"]["short"], case["want"]["short"]
    ctx = hip.Context(0)
    try:
        def refused(sp, out_bytes=None, rc=EINVAL):
            sp = np.array(sp, dtype=np.uint32).reshape(-1, 4)
            n = int(sp[:, 2].astype(np.uint64).sum()) if out_bytes is None else out_bytes
            out = np.full(max(n, 0) + 64, 0xA5, dtype=np.uint8)
            assert _raw_spell(ctx, sp, out, n) == rc, sp
            assert (out == 0xA5).all(), "a refused call wrote to the output"

        def works():
            assert (ctx.spell(good) == want).all()

        refused(good)                                           # no table
        ctx.set_bases(bases, base_off)
        works()
        n = len(LENGTHS)
        for bad in ([(n, 0, 1, 0)],                             # source = n_sources
                    [(0, 0, 1, 0), (4, 60, 4, 0)],              # first + len one beyond the source
                    [(4, 63, 1, 1)],
                    [(BIG, 0xFFFFFFFF, 2, 0)],                  # first + len wraps 32 bits
                    [(BIG, 0xFFFFFFF0, 0x20, 1)],
                    [(4, 0, 10, 2)]):                           # rc = 2
            refused(bad)
            works()
        for d in (-1, 1):                                       # out_bytes one off
            refused(good, len(want) + d)
            works()
        info = ctx.spell_info()
        # tables that are refused: the one that is there stays
        for off in (base_off[::-1].copy(), np.concatenate([base_off[:3], [base_off[2] - 1], base_off[3:]]), base_off + np.uint64(1)):
            off = np.ascontiguousarray(off, dtype=np.uint64)
            assert ctx.L.rala_hip_set_bases(ctx.h, bases.ctypes.data, off.ctypes.data, len(off) - 1, hip.MEM_HOST) == EINVAL
            works()
        assert ctx.spell_info()["sources"] == info["sources"] == len(LENGTHS)
    finally:
        ctx.close()


def test_table_replaced_released_and_independent_of_the_piles(case):
    bases, base_off = case["bases"], case["base_off"]
    ctx = hip.Context(0)
    try:
        ctx.set_bases(bases, base_off)
        other, other_off = spans.pack([b"GATTACA" * 9, b"", b"NNNNACGTacgt"])
        ctx.set_bases(other, other_off)
        sp = np.array([(0, 1, 62, 1), (1, 0, 0, 0), (2, 0, 12, 1), (2, 3, 5, 0)], dtype=np.uint32)
        assert (ctx.spell(sp) == spans.spell(other, other_off, sp)).all()
        assert ctx.spell_info()["sources"] == 3 and ctx.spell_info()["source_bytes"] == len(other)
        out = np.full(64, 0xA5, dtype=np.uint8)
        assert _raw_spell(ctx, [(3, 0, 1, 0)], out, 1) == EINVAL          # (a source of the table before)
        # the table does not care about the reads and the piles
        ds = Dataset.config("c1")
        ctx.set_reads(ds.read_len)
        ctx.set_overlaps(ds.overlaps)
        ctx.initialize()
        ctx.construct()
        assert len(ctx.graph()["node_read"]) > 0
        assert (ctx.spell(sp) == spans.spell(other, other_off, sp)).all()
        # device memory as input
        rt = hip._hip_runtime()
        p = ctypes.c_void_p()
        assert rt.hipMalloc(ctypes.byref(p), len(bases)) == 0
        try:
            assert rt.hipMemcpy(p, bases.ctypes.data, len(bases), 1) == 0
            ctx.set_bases(None, base_off, device_ptr=p)
        finally:
            rt.hipFree(p)                                           # (the context holds a copy)
        for name in ("short", "three_tiles"):
            assert (ctx.spell(case["lists"][name]) == case["want"][name]).all()
        # released
        ctx.set_bases(None, np.zeros(0, dtype=np.uint64))
        assert ctx.spell_info()["sources"] == 0
        assert _raw_spell(ctx, [(0, 0, 1, 0)], out, 1) == EINVAL and (out == 0xA5).all()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    return host.synthetic_reads(tmp=tmp_path_factory.mktemp("synth"))


@pytest.mark.parametrize("kind", ["fasta", "fasta_bgzf", "fastq_gzip"])
def test_keep_bases_leaves_the_gathered_reads_as_the_table(reads, tmp_path, kind):
    fastq = kind.startswith("fastq")
    text = host.fastq_text(reads) if fastq else host.fasta_text(reads, 60)
    blob = {"fasta": text, "fasta_bgzf": host.bgzf(text, list(range(20_000, len(text), 20_000))), "fastq_gzip": gzip.compress(text, 6)}[kind]
    path = str(tmp_path / ("reads.fastq.gz" if fastq else "reads.fasta.gz" if kind.endswith("bgzf") else "reads.fasta"))
    open(path, "wb").write(blob)
    ctx = hip.Context(0)
    try:
        ctx.set_option("gzip_on_device", 1)
        irregular, ix = ctx.index_sequences(path, fastq)
        assert irregular == 0 and len(ix["names"]) == len(reads) > 200
        wanted = np.array([k for k in range(len(reads)) if k % 3 != 1], dtype=np.uint64)
        plain = ctx.slice_sequences(path, wanted, ix["length"])
        assert plain[0] == 0 and ctx.spell_info()["sources"] == 0           # without the option: no table
        ctx.set_option("keep_bases", 1)
        irregular, none, base_off = ctx.slice_sequences(path, wanted, ix["length"], host_copy=False)
        assert irregular == 0 and none is None
        info = ctx.spell_info()
        assert info["from_slice"] == 1 and info["sources"] == len(wanted) and info["source_bytes"] == int(base_off[-1])
        # identity spans spell the wanted reads, which are the file's
        lens = np.diff(base_off.astype(np.int64))
        ident = np.stack([np.arange(len(wanted)), np.zeros(len(wanted)), lens, np.zeros(len(wanted))], axis=1).astype(np.uint32)
        got = ctx.spell(ident)
        want = np.frombuffer(b"".join(reads[int(k)][1] for k in wanted), dtype=np.uint8)
        assert (got == want).all() and (got == plain[1]).all()
        # trimmed and reverse spans
        rng = np.random.default_rng(5)
        first = (rng.random(len(wanted)) * lens * 0.4).astype(np.int64)
        take = np.maximum(0, ((lens - first) * rng.random(len(wanted))).astype(np.int64))
        sp = np.stack([np.arange(len(wanted)), first, take, rng.integers(0, 2, len(wanted))], axis=1).astype(np.uint32)
        sp = sp[rng.permutation(len(sp))]
        assert (ctx.spell(sp) == spans.spell(want, base_off, sp)).all()
        # with a host buffer as well: the copy is what it is without the option, and the table is there
        both = ctx.slice_sequences(path, wanted, ix["length"])
        assert both[0] == 0 and (both[1] == plain[1]).all() and ctx.spell_info()["from_slice"] == 1
        assert (ctx.spell(sp) == spans.spell(want, base_off, sp)).all()
        # the file is cut short between the passes: refused, and no table is left
        open(path, "wb").write(blob[:len(blob) * 2 // 3])
        assert ctx.slice_sequences(path, wanted, ix["length"], host_copy=False)[0] != 0
        assert ctx.spell_info()["sources"] == 0
        out = np.full(64, 0xA5, dtype=np.uint8)
        assert _raw_spell(ctx, ident[:1], out, int(lens[0])) == EINVAL
    finally:
        ctx.close()
