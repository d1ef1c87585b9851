"""CPU: the host side of the sequence index - the shim over io::read_fasta / io::read_fastq (rala_amd/host/io_capi.cpp: names,
lengths and a hash of every read's bases, the verdict of every sequence test), the exports of the device entry points, and the
second pass's slicer (io::slice_sequences), which cuts the reads' bases out of a plain or a BGZF file with an index.  The index
here is built in Python from the text; the lengths in it are the host reader's."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

from rala_amd import build, hip
from rala_amd.synth import Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    build.build_host()
    L = ctypes.CDLL(os.path.join(ROOT, "rala_amd", "host", "libassembly_graph.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.io_seq_parse.restype = vp
    L.io_seq_parse.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.io_seq_ok.argtypes = [vp]
    L.io_seq_size.restype = u64
    L.io_seq_size.argtypes = [vp]
    L.io_seq_name_bytes.restype = u64
    L.io_seq_name_bytes.argtypes = [vp]
    L.io_seq_copy.argtypes = [vp] * 5
    L.io_seq_free.argtypes = [vp]
    L.io_seq_slice.argtypes = [ctypes.c_char_p, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, ctypes.c_uint32, vp, vp]
    return L


def fnv(data):
    h = 0xcbf29ce484222325
    for c in data:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def host_read(path, fastq):
    """what io::read_fasta / io::read_fastq give: names (bytes), length, hash of the bases"""
    L = _lib()
    h = L.io_seq_parse(os.fsencode(path), int(fastq))
    try:
        assert L.io_seq_ok(h)
        n, nb = int(L.io_seq_size(h)), int(L.io_seq_name_bytes(h))
        arena = np.zeros(max(nb, 1), dtype=np.uint8)
        name_len, length = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        hashes = np.zeros(n, dtype=np.uint64)
        L.io_seq_copy(h, arena.ctypes.data, name_len.ctypes.data, length.ctypes.data, hashes.ctypes.data)
        raw, names, at = arena.tobytes(), [], 0
        for k in name_len:
            names.append(raw[at:at + int(k)])
            at += int(k)
        return {"names": names, "length": length, "hash": hashes}
    finally:
        L.io_seq_free(h)


def member(data, level=6):
    """one BGZF member (tests/test_gpu_bgzf.py's layout)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    total = 18 + len(body) + 8
    assert total <= 65536
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1) +
            body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf(data, cuts, eof=True, empty_at=()):
    """data as BGZF members that end at the text offsets `cuts` (and at most 60000 bytes of text each); empty_at: the
    numbers of the members in front of which an empty member is put"""
    edges = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out, lo, k = [], 0, 0
    for hi in edges:
        while lo < hi:
            if k in empty_at:
                out.append(member(b""))
            n = min(hi - lo, 60000)
            out.append(member(data[lo:lo + n]))
            lo += n
            k += 1
    if eof:
        out.append(member(b""))
    return b"".join(out)


def bgzf_members(blob):
    """rala_hip_bgzf_index's arrays (no device): file offsets, sizes, text sizes, text offsets"""
    L = hip.lib()
    L.rala_hip_bgzf_index.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 6
    n, valid = ctypes.c_uint64(0), ctypes.c_int(0)
    assert L.rala_hip_bgzf_index(blob, len(blob), 0, 0, ctypes.byref(n), None, None, None, None, ctypes.byref(valid)) == 0
    assert valid.value == 1
    m = n.value
    off, text_off = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    comp, text = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    assert L.rala_hip_bgzf_index(blob, len(blob), 0, m, ctypes.byref(n), off.ctypes.data, comp.ctypes.data, text.ctypes.data,
                                 text_off.ctypes.data, ctypes.byref(valid)) == 0
    return {"off": off, "bytes": comp, "text_bytes": text, "text_off": text_off}


def slice_reads(path, index, wanted, members=None, threads=3):
    """io::slice_sequences -> (hashes, numbers of bases) of the wanted reads, or None when it refuses"""
    L = _lib()
    off = np.ascontiguousarray(index["data_off"], dtype=np.uint64)
    span = np.ascontiguousarray(index["data_span"], dtype=np.uint64)
    length = np.ascontiguousarray(index["length"], dtype=np.uint32)
    wanted = np.ascontiguousarray(wanted, dtype=np.uint64)
    hashes, bases = np.zeros(len(wanted), dtype=np.uint64), np.zeros(len(wanted), dtype=np.uint32)
    m = members or {"off": np.zeros(0, np.uint64), "bytes": np.zeros(0, np.uint32), "text_bytes": np.zeros(0, np.uint32),
                    "text_off": np.zeros(0, np.uint64)}
    ok = L.io_seq_slice(os.fsencode(path), len(off), off.ctypes.data, span.ctypes.data, length.ctypes.data, len(m["off"]),
                        m["off"].ctypes.data, m["bytes"].ctypes.data, m["text_bytes"].ctypes.data, m["text_off"].ctypes.data,
                        wanted.ctypes.data, len(wanted), threads, hashes.ctypes.data, bases.ctypes.data)
    return (hashes, bases) if ok else None


def python_index(text, fastq):
    """data_off / data_span of every record of a FASTA text or a four-line FASTQ text"""
    off, span = [], []
    if fastq:
        starts = [0] + [i + 1 for i in range(len(text)) if text[i:i + 1] == b"\n" and i + 1 < len(text)]
        assert len(starts) % 4 == 0
        for r in range(len(starts) // 4):
            off.append(starts[4 * r + 1])
            span.append(starts[4 * r + 2] - starts[4 * r + 1])
    else:
        rec = [i for i in range(len(text)) if text[i:i + 1] == b">" and (i == 0 or text[i - 1:i] == b"\n")]
        for k, p in enumerate(rec):
            nl = text.find(b"\n", p)
            d = len(text) if nl < 0 else nl + 1
            off.append(d)
            span.append((rec[k + 1] if k + 1 < len(rec) else len(text)) - d)
    return {"data_off": np.array(off, dtype=np.uint64), "data_span": np.array(span, dtype=np.uint64)}


def synthetic_reads(n_reads=300, genome=40_000, seed=3, tmp=None):
    """(name, bases) of a synthetic set (rala_amd.synth writes two lines per read)"""
    ds = Dataset(n_reads, genome, seed)
    path = os.path.join(str(tmp), "synth.fasta")
    ds.write_fasta(path)
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[2 * i][1:], lines[2 * i + 1]) for i in range(ds.n_reads)]


def fasta_text(reads, width, eol=b"\n"):
    out = []
    for name, seq in reads:
        out.append(b">" + name + eol)
        if width:
            out.extend(seq[i:i + width] + eol for i in range(0, len(seq), width))
        else:
            out.append(seq + eol)
    return b"".join(out)


def fastq_text(reads, eol=b"\n"):
    return b"".join(b"@" + name + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol for name, seq in reads)


AWKWARD_FASTA = {
    "crlf": b">a desc\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
    "lone_cr": b">a\nAC\rGT\nA\r\rC\r\r\n>b\rx y\nTT\n",
    "no_final_newline": b">a\nACGT\n>b\nGGC",
    "cr_at_the_end": b">a\nACGT\n>b\nGGC\r",
    "header_last": b">a\nAC\n>b",
    "header_last_cr": b">a\nAC\n>b\r",
    "header_last_newline": b">a\nAC\n>b\n",
    "lengths_0_and_1": b">e\n>one\nA\n>e2\n\n>t\nAC\n",
    "empty_name": b">\nACGT\n> desc\nAA\n>\tx\nC\n",
    "descriptions": b">a b c\nAC\n>d\te f\nGT\n>g \nTT\n",
    "blank_lines": b">a\nAC\n\nGT\n\r\n\n>b\n\nA\n\n",
    "text_in_front": b"junk line\n;comment\nAC>GT\n>a\nAC\n>b\nG>T\n",
    "gt_inside": b">a>b\nAC>\n>\n>c\n",
    "empty_file_but_newline": b"\n",
}
AWKWARD_FASTQ = {
    "plain": b"@a\nACGT\n+\nIIII\n@b x\nGG\n+\nII\n",
    "crlf": b"@a d\r\nACGT\r\n+\r\nIIII\r\n@b\r\nGG\r\n+\r\nII\r\n",
    "no_final_newline": b"@a\nACGT\n+\nIIII\n@b\nGG\n+\nII",
    "quality_first_bytes": b"@a\nACGT\n+\n@III\n@b\nGG\n+\n+I\n@c\nTTT\n+\n>>>\n",
    "plus_name": b"@a\nACGT\n+a\nIIII\n@b\nGG\n+b some\nII\n",
    "lone_cr": b"@a\nAC\rT\n+\nIIII\n@b\rz\nGG\n+\nII\n",
    "empty_sequence": b"@a\n\n+\n\n@b\nGG\n+\nII\n",
    "length_1": b"@a\nA\n+\nI\n@\nC\n+\nI\n",
    "no_at": b"a\nACGT\n+\nIIII\n>b\nGG\n+\nII\n",
}


@pytest.mark.parametrize("name", sorted(AWKWARD_FASTA))
def test_shim_and_slicer_on_handmade_fasta(tmp_path, name):
    text = AWKWARD_FASTA[name]
    path = str(tmp_path / "x.fasta")
    open(path, "wb").write(text)
    got = host_read(path, False)
    # the same records through Python's own reading of Lines::next: lines end at a newline, one carriage return in front
    # of it goes; the file's last line keeps its own
    lines = text.split(b"\n")
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    want = []
    for l in lines:
        if l.startswith(b">"):
            tok = l[1:].replace(b"\t", b" ").split(b" ")[0]
            want.append([tok, b""])
        elif want:
            want[-1][1] += l
    assert got["names"] == [w[0] for w in want]
    assert got["length"].tolist() == [len(w[1]) for w in want]
    assert got["hash"].tolist() == [fnv(w[1]) for w in want]
    ix = python_index(text, False)
    ix["length"] = got["length"]
    if len(want):
        hashes, bases = slice_reads(path, ix, np.arange(len(want)))
        assert bases.tolist() == got["length"].tolist() and hashes.tolist() == got["hash"].tolist()


@pytest.mark.parametrize("name", sorted(AWKWARD_FASTQ))
def test_shim_and_slicer_on_handmade_fastq(tmp_path, name):
    text = AWKWARD_FASTQ[name]
    path = str(tmp_path / "x.fastq")
    open(path, "wb").write(text)
    got = host_read(path, True)
    lines = text.split(b"\n")
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    assert len(lines) % 4 == 0
    want = [(lines[k][1:].replace(b"\t", b" ").split(b" ")[0], lines[k + 1]) for k in range(0, len(lines), 4)]
    assert got["names"] == [w[0] for w in want]
    assert got["length"].tolist() == [len(w[1]) for w in want]
    assert got["hash"].tolist() == [fnv(w[1]) for w in want]
    ix = python_index(text, True)
    ix["length"] = got["length"]
    hashes, bases = slice_reads(path, ix, np.arange(len(want)))
    assert bases.tolist() == got["length"].tolist() and hashes.tolist() == got["hash"].tolist()


def test_entry_points_are_exported_and_bound():
    L = hip.lib()
    for name in ("rala_hip_index_sequences", "rala_hip_get_sequence_index", "rala_hip_get_sequence_timings"):
        assert hasattr(L, name) and name in hip.SYMBOLS
    assert L.rala_hip_index_sequences.argtypes is not None and len(L.rala_hip_index_sequences.argtypes) == 7
    assert callable(hip.Context.index_sequences) and callable(hip.Context.sequence_timings)


@pytest.mark.parametrize("shape", ["fasta1", "fasta60", "fasta0", "fasta80crlf", "fastq", "fastqcrlf"])
def test_slicer_on_synthetic_sets_plain_and_bgzf(tmp_path, shape):
    reads = synthetic_reads(tmp=tmp_path)
    fastq = shape.startswith("fastq")
    eol = b"\r\n" if shape.endswith("crlf") else b"\n"
    text = fastq_text(reads, eol) if fastq else fasta_text(reads, int(shape[5:].replace("crlf", "")), eol)
    plain = str(tmp_path / ("reads." + ("fastq" if fastq else "fasta")))
    open(plain, "wb").write(text)
    want = host_read(plain, fastq)
    assert want["names"] == [r[0] for r in reads] and want["hash"].tolist() == [fnv(r[1]) for r in reads]
    ix = python_index(text, fastq)
    ix["length"] = want["length"]
    rng = np.random.default_rng(7)
    some = np.sort(rng.choice(len(reads), len(reads) // 5, replace=False))
    for wanted in (np.arange(len(reads)), some, some[:1], np.zeros(0, dtype=np.uint64)):
        for threads in (1, 5):
            hashes, bases = slice_reads(plain, ix, wanted, threads=threads)
            assert bases.tolist() == want["length"][wanted.astype(int)].tolist()
            assert hashes.tolist() == want["hash"][wanted.astype(int)].tolist()
    # BGZF: members that end between a carriage return and its newline, in front of and behind newlines, of one byte
    cuts = []
    for k in range(0, len(text), 7919):
        nl = text.find(b"\n", k)
        if nl >= 0:
            cuts += [nl, nl + 1, nl + 2]
    blob = bgzf(text, cuts, empty_at=(2, 5))
    gz = plain + ".gz"
    open(gz, "wb").write(blob)
    assert host_read(gz, fastq)["hash"].tolist() == want["hash"].tolist()
    members = bgzf_members(blob)
    for wanted in (np.arange(len(reads)), some, some[-1:]):
        hashes, bases = slice_reads(gz, ix, wanted, members, threads=4)
        assert bases.tolist() == want["length"][wanted.astype(int)].tolist()
        assert hashes.tolist() == want["hash"][wanted.astype(int)].tolist()


def test_slicer_refuses_an_index_that_is_not_the_files(tmp_path):
    text = b">a\nACGT\n>b\nGG\n"
    path = str(tmp_path / "x.fasta")
    open(path, "wb").write(text)
    ix = python_index(text, False)
    ix["length"] = np.array([4, 2], dtype=np.uint32)
    assert slice_reads(path, ix, [0, 1]) is not None
    ix["length"] = np.array([4, 3], dtype=np.uint32)
    assert slice_reads(path, ix, [0, 1]) is None
    ix["length"] = np.array([4, 2], dtype=np.uint32)
    ix["data_span"] = np.array([5, 300], dtype=np.uint64)
    assert slice_reads(path, ix, [0, 1]) is None
    assert slice_reads(str(tmp_path / "missing.fasta"), ix, [0]) is None
