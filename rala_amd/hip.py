"""ctypes binding of librala_hip's C ABI (include/rala_hip.h).

Used by the tests and by bench.py.  There is no fallback of any kind: if the shared
library is missing or no HIP device is usable, construction raises.
"""
import ctypes
import os

import numpy as np

from . import build as _build

TYPE_X, TYPE_A, TYPE_B, TYPE_AB, TYPE_BA = range(5)
NO_READ = 0xFFFFFFFF
MEM_HOST, MEM_DEVICE, MEM_HOST_ASYNC = 0, 1, 2

ERRORS = {0: "OK", -1: "EDEVICE", -2: "EINVAL", -3: "ECAPACITY", -4: "EFILTERED", -5: "ENOMEM", -6: "ENOTAFILE", -7: "ETOOLARGE"}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "librala_hip.so")

# every symbol include/rala_hip.h declares
SYMBOLS = (
    "rala_hip_create", "rala_hip_destroy", "rala_hip_last_error", "rala_hip_set_option", "rala_hip_stream",
    "rala_hip_set_reads", "rala_hip_set_overlaps", "rala_hip_initialize", "rala_hip_construct",
    "rala_hip_remove_transitive_edges", "rala_hip_tr_mark", "rala_hip_get_valid", "rala_hip_get_piles",
    "rala_hip_get_pile_data", "rala_hip_get_pile_row_digests", "rala_hip_get_pile_rows_info", "rala_hip_get_intervals", "rala_hip_get_overlaps", "rala_hip_get_graph_size",
    "rala_hip_get_graph", "rala_hip_get_timings", "rala_hip_get_num_prefiltered",
    "rala_hip_dedupe", "rala_hip_emit_bound_tuples", "rala_hip_set_bound_tuples", "rala_hip_import_state",
    "rala_hip_emit_bound_tuples_bucketed", "rala_hip_get_device_state", "rala_hip_import_state_device",
    "rala_hip_bound_records_fit", "rala_hip_emit_bound_records_bucketed", "rala_hip_set_bound_records",
    "rala_hip_copy_device_state", "rala_hip_layout", "rala_hip_layout_batch", "rala_hip_get_layout_info",
    "rala_hip_find_repetitive_hills",
    "rala_hip_mg_unique_id", "rala_hip_mg_local_group_create", "rala_hip_mg_local_group_destroy", "rala_hip_mg_create",
    "rala_hip_mg_create_contexts", "rala_hip_mg_join", "rala_hip_set_name_table", "rala_hip_set_overlaps_from_paf", "rala_hip_set_overlaps_from_mhap",
    "rala_hip_get_ingest_timings", "rala_hip_get_inflate_timings", "rala_hip_get_gzip_timings", "rala_hip_gzip_head", "rala_hip_gzip_chain", "rala_hip_gzip_chain_members", "rala_hip_gzip_find_members", "rala_hip_get_gzip_members",
    "rala_hip_gzip_pieces", "rala_hip_gzip_compose_windows", "rala_hip_get_gzip_pieces_info", "rala_hip_gzip_compose_windows_masked", "rala_hip_gzip_members_proof",
    "rala_hip_get_gzip_member_pieces_info", "rala_hip_mg_tokenise_sensitive", "rala_hip_bgzf_index", "rala_hip_get_overlap_columns", "rala_hip_tokenise_sensitive_paf",
    "rala_hip_bgzf_index_range", "rala_hip_bgzf_pieces_chain", "rala_hip_tokenise_sensitive", "rala_hip_mg_set_overlaps_from_mhap",
    "rala_hip_mg_set_overlaps_from_paf", "rala_hip_mg_get_slice",
    "rala_hip_index_sequences", "rala_hip_get_sequence_index", "rala_hip_get_sequence_timings",
    "rala_hip_build_name_table", "rala_hip_get_name_table", "rala_hip_copy_name_table", "rala_hip_name_hash",
    "rala_hip_get_name_table_info",
    "rala_hip_slice_sequences", "rala_hip_get_sequence_slice_info", "rala_hip_crc32_chain",
    "rala_hip_set_bases", "rala_hip_spell", "rala_hip_get_spell_info",
    "rala_hip_mg_destroy", "rala_hip_mg_last_error", "rala_hip_mg_set_reads", "rala_hip_mg_slice_cuts",
    "rala_hip_mg_set_overlaps", "rala_hip_mg_run", "rala_hip_mg_run_threads", "rala_hip_mg_context",
    "rala_hip_mg_owner_context",
    "rala_hip_mg_get_pile_data", "rala_hip_mg_get_pile_row_digests", "rala_hip_mg_get_timings",
    "rala_hip_layout_split", "rala_hip_mg_layout_batch", "rala_hip_mg_layout_batch_threads", "rala_hip_mg_get_layout_info",
)
COMM_RCCL, COMM_LOCAL = 0, 1


class OverlapsC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("a_id", "b_id", "a_begin", "a_end", "b_begin", "b_end", "length", "strand")]


class DeviceState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("begin", "end", "median", "p10", "alive", "n_pits", "n_hills", "slot",
                                               "pool")] + [("pool_count", ctypes.c_uint64), ("valid", ctypes.c_void_p)]


class Timings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in
                ("dedupe_ms", "bucket_ms", "pile_ms", "classify_ms", "death_ms", "finish_ms", "tail_host_ms",
                 "tr_ms", "total_ms")] + [("pile_launches", ctypes.c_uint32), ("death_rounds", ctypes.c_uint32),
                                  ("pile_overflow_reads", ctypes.c_uint32),
                                  ("pile_position_reads", ctypes.c_uint32),
                                  ("pile_unbounded_reads", ctypes.c_uint32), ("pool_regrown", ctypes.c_uint32),
                                  ("repeats_ms", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MgTimings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("emit_ms", "exchange_ms", "owner_ms", "gather_ms", "construct_ms",
                                              "repeats_ms", "tr_ms", "total_ms")] + [("tuples_sent", ctypes.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class IngestTimings(ctypes.Structure):
    """rala_hip_ingest_timings"""
    _fields_ = [("ship_ms", ctypes.c_float), ("tokenize_ms", ctypes.c_float), ("bytes", ctypes.c_uint64), ("lines", ctypes.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GzipTimings(ctypes.Structure):
    """rala_hip_gzip_timings"""
    _fields_ = [(n, ctypes.c_float) for n in ("find_ms", "decode_ms", "resolve_ms")] + [(n, ctypes.c_uint64) for n in (
        "compressed_bytes", "text_bytes", "chunks", "chunks_with_candidate", "chunks_confirmed", "chunks_refuted",
        "max_wave_text_bytes")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GzipPiecesInfo(ctypes.Structure):
    """rala_hip_gzip_pieces_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("own_chunks", "own_jobs", "halo_jobs", "own_text_bytes", "window_markers")] + [
        ("longest_chase", ctypes.c_uint32), ("compose_ms", ctypes.c_float), ("exchange_ms", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GzipMemberPiecesInfo(ctypes.Structure):
    """rala_hip_gzip_member_pieces_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("own_candidates", "members_begun", "member_ends")] + [
        ("registers_sent", ctypes.c_uint32), ("floor_stops", ctypes.c_uint32), ("compose_ms", ctypes.c_float), ("pad", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


GZIP_WINDOW = 32768
GZIP_NOTHING = 0x4000       # RALA_HIP_GZIP_NOTHING


class LayoutInfo(ctypes.Structure):
    _fields_ = [("components_fused_256", ctypes.c_uint32), ("components_fused_1024", ctypes.c_uint32),
                ("components_stepped", ctypes.c_uint32), ("components_empty", ctypes.c_uint32),
                ("points_fused_256", ctypes.c_uint64), ("points_fused_1024", ctypes.c_uint64),
                ("points_stepped", ctypes.c_uint64), ("step_tiles", ctypes.c_uint32), ("launches", ctypes.c_uint32),
                ("device_ms", ctypes.c_float)]


class MgLayoutInfo(ctypes.Structure):
    """rala_hip_mg_layout_info"""
    _fields_ = [(n, ctypes.c_uint32) for n in ("first_point", "end_point", "components_fused_256", "components_fused_1024",
                                               "step_tiles", "launches", "gathers")] + [
        (n, ctypes.c_uint64) for n in ("cost", "total_cost", "bytes_received")] + [
        ("device_ms", ctypes.c_float), ("exchange_ms", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class NameTableInfo(ctypes.Structure):
    """rala_hip_name_table_info"""
    _fields_ = [("names", ctypes.c_uint64), ("distinct", ctypes.c_uint64), ("n_buckets", ctypes.c_uint64),
                ("longest_probe", ctypes.c_uint32), ("device_ms", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SequenceSliceInfo(ctypes.Structure):
    """rala_hip_sequence_slice_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("windows", "max_window_text_bytes", "bases")] + [(n, ctypes.c_float) for n in (
        "ship_ms", "kernel_ms", "gather_ms", "copy_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SpellInfo(ctypes.Structure):
    """rala_hip_spell_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("sources", "source_bytes", "spans", "bytes", "windows", "launches")] + [(n, ctypes.c_float) for n in (
        "upload_ms", "kernel_ms", "copy_ms")] + [("from_slice", ctypes.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib = None


def name_hash(name):
    """rala_hip_name_hash: the name table's hash of a name (bytes), on the host - no context, no device"""
    name = bytes(name)
    return int(lib().rala_hip_name_hash(ctypes.c_char_p(name), len(name)))


def lib(build=True):
    """Load librala_hip.so (building it in-tree first when sources are newer)."""
    global _lib
    if _lib is None:
        path = LIB_PATH
        if build:
            path = _build.build_hip()
        if os.environ.get("RALA_HIP_LIB_AB"):        # (measurements: another build of the library, profiles/r19_pipeline_split.txt)
            path = os.environ["RALA_HIP_LIB_AB"]
        if not os.path.exists(path):
            raise RuntimeError("librala_hip.so is missing: run __graft_entry__.build()")
        L = ctypes.CDLL(path)
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        L.rala_hip_create.argtypes = [i32, ctypes.POINTER(vp)]
        L.rala_hip_destroy.argtypes = [vp]
        L.rala_hip_destroy.restype = None
        L.rala_hip_last_error.argtypes = [vp]
        L.rala_hip_last_error.restype = ctypes.c_char_p
        L.rala_hip_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
        L.rala_hip_stream.argtypes = [vp]
        L.rala_hip_stream.restype = vp
        L.rala_hip_set_reads.argtypes = [vp, vp, u64]
        L.rala_hip_set_overlaps.argtypes = [vp, ctypes.POINTER(OverlapsC), u64, i32]
        L.rala_hip_initialize.argtypes = [vp]
        L.rala_hip_construct.argtypes = [vp, ctypes.POINTER(OverlapsC), u64]
        L.rala_hip_remove_transitive_edges.argtypes = [vp, ctypes.POINTER(u32)]
        L.rala_hip_tr_mark.argtypes = [vp, u32, u32, vp, vp, vp, vp, ctypes.POINTER(u32)]
        L.rala_hip_get_valid.argtypes = [vp, vp]
        L.rala_hip_get_piles.argtypes = [vp, vp, vp, vp, vp, vp]
        L.rala_hip_get_pile_data.argtypes = [vp, u64, vp]
        L.rala_hip_get_pile_row_digests.argtypes = [vp, vp, vp, vp]
        L.rala_hip_get_pile_rows_info.argtypes = [vp, vp, vp]
        L.rala_hip_get_intervals.argtypes = [vp, i32, vp, vp, vp]
        L.rala_hip_get_overlaps.argtypes = [vp, i32, ctypes.POINTER(u64), vp, vp, vp, vp, vp, vp, vp]
        L.rala_hip_get_graph_size.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.rala_hip_get_graph.argtypes = [vp, vp, vp, vp, vp, vp]
        L.rala_hip_get_timings.argtypes = [vp, ctypes.POINTER(Timings)]
        L.rala_hip_get_num_prefiltered.argtypes = [vp, ctypes.POINTER(u64)]
        L.rala_hip_dedupe.argtypes = [vp]
        L.rala_hip_emit_bound_tuples.argtypes = [vp, vp]
        L.rala_hip_set_bound_tuples.argtypes = [vp, vp, u64, i32]
        L.rala_hip_import_state.argtypes = [vp] + [vp] * 11
        L.rala_hip_emit_bound_tuples_bucketed.argtypes = [vp, u32, vp, vp]
        L.rala_hip_get_device_state.argtypes = [vp, ctypes.POINTER(DeviceState)]
        L.rala_hip_import_state_device.argtypes = [vp, ctypes.POINTER(DeviceState)]
        L.rala_hip_copy_device_state.argtypes = [vp, ctypes.POINTER(DeviceState)]
        L.rala_hip_layout.argtypes = [vp, u32, vp, vp, vp, vp, u32, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        L.rala_hip_layout_batch.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, ctypes.c_double, ctypes.c_double]
        L.rala_hip_get_layout_info.argtypes = [vp, ctypes.POINTER(LayoutInfo)]
        L.rala_hip_find_repetitive_hills.argtypes = [vp, u64, u32, u32, ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint16]
        L.rala_hip_mg_unique_id.argtypes = [vp]
        L.rala_hip_mg_local_group_create.argtypes = [u32, ctypes.POINTER(vp)]
        L.rala_hip_mg_local_group_destroy.argtypes = [vp]
        L.rala_hip_mg_local_group_destroy.restype = None
        L.rala_hip_mg_create.argtypes = [i32, u32, u32, i32, vp, ctypes.POINTER(vp)]
        L.rala_hip_mg_create_contexts.argtypes = [i32, u32, u32, ctypes.POINTER(vp)]
        L.rala_hip_mg_join.argtypes = [vp, i32, vp]
        L.rala_hip_mg_destroy.argtypes = [vp]
        L.rala_hip_mg_destroy.restype = None
        L.rala_hip_mg_last_error.argtypes = [vp]
        L.rala_hip_mg_last_error.restype = ctypes.c_char_p
        L.rala_hip_mg_set_reads.argtypes = [vp, vp, u64]
        L.rala_hip_mg_slice_cuts.argtypes = [vp, vp, u64, u32, vp]
        L.rala_hip_mg_set_overlaps.argtypes = [vp, ctypes.POINTER(OverlapsC), u64, u64, i32]
        L.rala_hip_mg_run.argtypes = [vp, ctypes.POINTER(OverlapsC), u64, ctypes.POINTER(u32)]
        L.rala_hip_mg_run_threads.argtypes = [vp, u32, vp, vp, ctypes.POINTER(u32)]
        L.rala_hip_mg_context.argtypes = [vp]
        L.rala_hip_mg_context.restype = vp
        L.rala_hip_mg_owner_context.argtypes = [vp]
        L.rala_hip_mg_owner_context.restype = vp
        L.rala_hip_mg_get_pile_data.argtypes = [vp, u64, vp]
        L.rala_hip_mg_get_pile_row_digests.argtypes = [vp, vp, vp, vp]
        L.rala_hip_mg_get_timings.argtypes = [vp, ctypes.POINTER(MgTimings)]
        L.rala_hip_get_gzip_timings.argtypes = [vp, ctypes.POINTER(GzipTimings)]
        L.rala_hip_gzip_head.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(i32)]
        L.rala_hip_index_sequences.argtypes = [vp, ctypes.c_char_p, i32, u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(i32)]
        L.rala_hip_get_sequence_index.argtypes = [vp] + [vp] * 6
        L.rala_hip_get_sequence_timings.argtypes = [vp, ctypes.POINTER(IngestTimings)]
        L.rala_hip_set_name_table.argtypes = [vp, vp, u64, vp, u64]
        L.rala_hip_build_name_table.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.rala_hip_get_name_table.argtypes = [vp, vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.rala_hip_copy_name_table.argtypes = [vp, vp]
        L.rala_hip_name_hash.argtypes = [vp, u64]
        L.rala_hip_name_hash.restype = u64
        L.rala_hip_get_name_table_info.argtypes = [vp, ctypes.POINTER(NameTableInfo)]
        L.rala_hip_set_overlaps_from_paf.argtypes = [vp, ctypes.c_char_p, i32, u32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(i32)]
        L.rala_hip_get_overlap_columns.argtypes = [vp, ctypes.POINTER(u64), vp, vp]
        L.rala_hip_slice_sequences.argtypes = [vp, ctypes.c_char_p, vp, u64, vp, vp, u32, ctypes.POINTER(i32)]
        L.rala_hip_get_sequence_slice_info.argtypes = [vp, ctypes.POINTER(SequenceSliceInfo)]
        L.rala_hip_set_bases.argtypes = [vp, vp, vp, u64, i32]
        L.rala_hip_spell.argtypes = [vp, vp, u64, vp, u64]
        L.rala_hip_get_spell_info.argtypes = [vp, ctypes.POINTER(SpellInfo)]
        L.rala_hip_crc32_chain.argtypes = [vp, vp, u64]
        L.rala_hip_crc32_chain.restype = u32
        L.rala_hip_gzip_chain.argtypes = [vp] * 6 + [u64, u64, u32, u64, ctypes.POINTER(u64)] + [vp] * 4 + [ctypes.POINTER(GzipTimings), ctypes.POINTER(i32)]
        L.rala_hip_gzip_chain_members.argtypes = ([vp] * 6 + [u64] + [vp] * 8 + [u64, u64, u32, u32, u64, ctypes.POINTER(u64)] + [vp] * 5 +
                                                  [u64, ctypes.POINTER(u64)] + [vp] * 3 + [ctypes.POINTER(GzipTimings), ctypes.POINTER(i32)])
        L.rala_hip_gzip_find_members.argtypes = [vp, vp, u64, u64, ctypes.POINTER(u64), vp, vp]
        L.rala_hip_get_gzip_members.argtypes = [vp, ctypes.POINTER(u64), u64, vp, vp, vp]
        L.rala_hip_gzip_pieces.argtypes = [vp, u64, u64, u64, u64, u32, vp]
        L.rala_hip_gzip_compose_windows.argtypes = [vp, u32, u32, vp, ctypes.POINTER(i32)]
        L.rala_hip_get_gzip_pieces_info.argtypes = [vp, ctypes.POINTER(GzipPiecesInfo)]
        L.rala_hip_gzip_compose_windows_masked.argtypes = [vp, u32, vp, u32, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.rala_hip_gzip_members_proof.argtypes = [vp, vp, vp, u64] + [vp] * 7 + [u32, ctypes.POINTER(u64), ctypes.POINTER(i32)]
        L.rala_hip_get_gzip_member_pieces_info.argtypes = [vp, ctypes.POINTER(GzipMemberPiecesInfo)]
        L.rala_hip_layout_split.argtypes = [u32, vp, u32, u32, vp, vp]
        L.rala_hip_mg_layout_batch.argtypes = [vp, u32] + [vp] * 8 + [u32, ctypes.c_double, ctypes.c_double]
        L.rala_hip_mg_layout_batch_threads.argtypes = [vp, u32, u32] + [vp] * 6 + [u32, ctypes.c_double, ctypes.c_double]
        L.rala_hip_mg_get_layout_info.argtypes = [vp, ctypes.POINTER(MgLayoutInfo)]
        _lib = L
    return _lib


class RalaHipError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("librala_hip: %s (%d): %s" % (ERRORS.get(code, "?"), code, text))
        self.code = code


class DeviceOverlaps:
    """overlap columns that lie in device memory (kept alive by the caller, e.g. torch tensors): name -> pointer.
    Accepted where a sensitive set is (Context.construct, ShardedRank.run, run_ranks) once the context's option
    sensitive_in_device_memory is 1."""

    def __init__(self, ptrs, n, keep=None):
        self.ptrs, self.n, self.keep = dict(ptrs), int(n), keep

    def __len__(self):
        return self.n

    @classmethod
    def from_host(cls, ov, device):
        """upload numpy columns to `device` (the HIP runtime directly: hipMalloc / hipMemcpy, freed with the object)"""
        rt = _hip_runtime()
        keep, ptrs = _DeviceBlocks(rt), {}
        _rt_check(rt.hipSetDevice(int(device)), "hipSetDevice")
        for name, _ in OverlapsC._fields_:
            arr = np.ascontiguousarray(getattr(ov, name))
            p = ctypes.c_void_p()
            _rt_check(rt.hipMalloc(ctypes.byref(p), max(1, arr.nbytes)), "hipMalloc")
            keep.blocks.append(p)
            if arr.nbytes:
                _rt_check(rt.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1), "hipMemcpy")        # hipMemcpyHostToDevice
            ptrs[name] = p.value
        return cls(ptrs, len(ov), keep)


_rt = None


def _hip_runtime():
    global _rt
    if _rt is None:
        lib()                           # (librala_hip.so has brought the runtime into the process)
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
            try:
                _rt = ctypes.CDLL(name)
                break
            except OSError:
                continue
        if _rt is None:
            raise RalaHipError(-2, "libamdhip64 not found")
        _rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _rt.hipFree.argtypes = [ctypes.c_void_p]
        _rt.hipSetDevice.argtypes = [ctypes.c_int]
    return _rt


def _rt_check(rc, what):
    if rc != 0:
        raise RalaHipError(-2, "%s failed (%d)" % (what, rc))


class _DeviceBlocks:
    def __init__(self, rt):
        self.rt, self.blocks = rt, []

    def __del__(self):
        try:
            for p in self.blocks:
                self.rt.hipFree(p)
        except Exception:
            pass


def _soa(ov):
    """OverlapsC over an object with numpy members a_id … strand (kept alive by the caller), or over DeviceOverlaps."""
    c = OverlapsC()
    if isinstance(ov, DeviceOverlaps):
        for name, _ in OverlapsC._fields_:
            setattr(c, name, ov.ptrs[name])
        return c
    for name, _ in OverlapsC._fields_:
        arr = getattr(ov, name)
        want = np.uint8 if name == "strand" else np.uint32
        assert arr.dtype == want and arr.flags["C_CONTIGUOUS"], name
        setattr(c, name, arr.ctypes.data)
    return c


class Context:
    """One librala_hip context = one data set on one GPU."""

    def __init__(self, device=0, _borrowed=None):
        self.L = lib()
        self._owned = _borrowed is None
        if _borrowed is not None:
            h = ctypes.c_void_p(_borrowed)
        else:
            h = ctypes.c_void_p()
            rc = self.L.rala_hip_create(device, ctypes.byref(h))
            if rc != 0:
                raise RalaHipError(rc, "no usable HIP device %d" % device)
        self.h = h
        self.n_reads = 0
        self.n_overlaps = 0
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            if self._owned:
                self.L.rala_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RalaHipError(rc, self.L.rala_hip_last_error(self.h).decode())

    def set_option(self, key, value):
        self._check(self.L.rala_hip_set_option(self.h, key.encode(), int(value)))

    def stream(self):
        return self.L.rala_hip_stream(self.h)

    # ---- inputs ----
    def set_reads(self, read_len):
        rl = np.ascontiguousarray(read_len, dtype=np.uint32)
        self.read_len = rl
        self.n_reads = int(rl.shape[0])
        self._check(self.L.rala_hip_set_reads(self.h, rl.ctypes.data, self.n_reads))

    def index_sequences(self, path, fastq=False, threads=4):
        """rala_hip_index_sequences + rala_hip_get_sequence_index -> (irregular, index); index (None when irregular): names (list of
        bytes), length, data_off, data_span.  The lengths are the context's reads afterwards."""
        n, nb, irregular = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        self._check(self.L.rala_hip_index_sequences(self.h, os.fsencode(path), 1 if fastq else 0, threads, ctypes.byref(n), ctypes.byref(nb),
                                                    ctypes.byref(irregular)))
        if irregular.value:
            return irregular.value, None
        name_off, data_off, data_span = (np.zeros(n.value, dtype=np.uint64) for _ in range(3))
        name_len, length = (np.zeros(n.value, dtype=np.uint32) for _ in range(2))
        arena = np.zeros(max(nb.value, 1), dtype=np.uint8)
        self._check(self.L.rala_hip_get_sequence_index(self.h, name_off.ctypes.data, name_len.ctypes.data, data_off.ctypes.data,
                                                       data_span.ctypes.data, length.ctypes.data, arena.ctypes.data))
        raw = arena.tobytes()
        names = [raw[int(o):int(o) + int(k)] for o, k in zip(name_off, name_len)]
        self.n_reads = n.value
        return 0, {"names": names, "name_off": name_off, "length": length, "data_off": data_off, "data_span": data_span}

    # ---- the name table (name_table.h: 32-byte buckets as a (n_buckets, 8) uint32 array, the names' bytes as a uint8 array) ----
    def build_name_table(self):
        """rala_hip_build_name_table: the table from the current sequence index, built and installed on the device
        -> (n_buckets, n_distinct)"""
        nb, nd = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.rala_hip_build_name_table(self.h, ctypes.byref(nb), ctypes.byref(nd)))
        return nb.value, nd.value

    def get_name_table(self):
        """rala_hip_get_name_table: the installed table -> (buckets, arena)"""
        nb, ab = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.rala_hip_get_name_table(self.h, None, None, ctypes.byref(nb), ctypes.byref(ab)))
        buckets = np.zeros((nb.value, 8), dtype=np.uint32)
        arena = np.zeros(max(ab.value, 1), dtype=np.uint8)
        self._check(self.L.rala_hip_get_name_table(self.h, buckets.ctypes.data, arena.ctypes.data, ctypes.byref(nb), ctypes.byref(ab)))
        return buckets, arena[:ab.value]

    def set_name_table(self, buckets, arena):
        """rala_hip_set_name_table: a table built elsewhere (the host's)"""
        buckets = np.ascontiguousarray(buckets, dtype=np.uint32)
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        self._check(self.L.rala_hip_set_name_table(self.h, buckets.ctypes.data, buckets.shape[0], arena.ctypes.data if len(arena) else None,
                                                   len(arena)))

    def copy_name_table_from(self, src):
        """rala_hip_copy_name_table: src's installed table into this context, device to device"""
        self._check(self.L.rala_hip_copy_name_table(self.h, src.h))

    def name_table_info(self):
        t = NameTableInfo()
        self._check(self.L.rala_hip_get_name_table_info(self.h, ctypes.byref(t)))
        return t.as_dict()

    def set_overlaps_from_paf(self, path, check_lengths=False, threads=2):
        """rala_hip_set_overlaps_from_paf with the installed name table -> (irregular, first read with a length mismatch or -1)"""
        bad, irregular = ctypes.c_int64(-1), ctypes.c_int(0)
        self._check(self.L.rala_hip_set_overlaps_from_paf(self.h, os.fsencode(path), int(check_lengths), threads, ctypes.byref(bad),
                                                          ctypes.byref(irregular)))
        return irregular.value, bad.value

    def overlap_columns(self):
        """rala_hip_get_overlap_columns: the context's overlaps as they lie on the device -> dict of columns"""
        n = ctypes.c_uint64(0)
        self._check(self.L.rala_hip_get_overlap_columns(self.h, ctypes.byref(n), None, None))
        names = ("a_id", "b_id", "a_begin", "a_end", "b_begin", "b_end", "length")
        cols = {f: np.zeros(max(n.value, 1), dtype=np.uint32) for f in names}
        strand = np.zeros(max(n.value, 1), dtype=np.uint8)
        ptrs = (ctypes.c_void_p * 7)(*[cols[f].ctypes.data for f in names])
        self._check(self.L.rala_hip_get_overlap_columns(self.h, ctypes.byref(n), ptrs, strand.ctypes.data))
        out = {f: cols[f][:n.value] for f in names}
        out["strand"] = strand[:n.value]
        return out

    def slice_sequences(self, path, wanted, length, threads=4, host_copy=True):
        """rala_hip_slice_sequences: the bases of the reads `wanted` (ascending records of the current index; length = the
        index's lengths) cut out of the file on the device -> (irregular, bases, base_off); bases (None when refused) is one
        uint8 array, read wanted[k]'s bases are bases[base_off[k]:base_off[k + 1]].  host_copy False (with the option
        keep_bases): `bases` is NULL - the bases stay on the device as the table of bases - and None comes back"""
        wanted = np.ascontiguousarray(wanted, dtype=np.uint64)
        base_off = np.zeros(len(wanted) + 1, dtype=np.uint64)
        np.cumsum(np.asarray(length, dtype=np.uint64)[wanted.astype(np.int64)], out=base_off[1:])
        bases = np.zeros(max(int(base_off[-1]), 1), dtype=np.uint8) if host_copy else None
        irregular = ctypes.c_int(0)
        self._check(self.L.rala_hip_slice_sequences(self.h, os.fsencode(path), wanted.ctypes.data, len(wanted), base_off.ctypes.data,
                                                    bases.ctypes.data if host_copy else None, threads, ctypes.byref(irregular)))
        if irregular.value or not host_copy:
            return irregular.value, None, base_off
        return 0, bases[:int(base_off[-1])], base_off

    # ---- node bases as spans: the table of bases and what spans of it spell ----
    def set_bases(self, bases, base_off, device_ptr=None):
        """rala_hip_set_bases: source s is bases[base_off[s]:base_off[s + 1]] (uint8 array; or device_ptr: the bytes lie in
        device memory there); no sources: the table is released"""
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n = max(len(base_off) - 1, 0)
        if device_ptr is not None:
            ptr, mem = device_ptr, MEM_DEVICE
        else:
            bases = np.zeros(0, dtype=np.uint8) if bases is None else np.ascontiguousarray(bases, dtype=np.uint8)
            ptr, mem = (bases.ctypes.data if len(bases) else None), MEM_HOST
        self._check(self.L.rala_hip_set_bases(self.h, ptr, base_off.ctypes.data if len(base_off) else None, n, mem))

    def spell(self, spans, out=None, out_bytes=None):
        """rala_hip_spell: spans an (n, 4) uint32 array of (source, first, len, rc) -> what they spell, one uint8 array (out: the
        array to fill, out_bytes: what to tell the call it holds - the tests of the refusals)"""
        spans = np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 4)
        total = int(spans[:, 2].astype(np.uint64).sum()) if out_bytes is None else int(out_bytes)
        if out is None:
            out = np.zeros(max(total, 1), dtype=np.uint8)
        self._check(self.L.rala_hip_spell(self.h, spans.ctypes.data if len(spans) else None, len(spans), out.ctypes.data, total))
        return out[:total]

    def spell_info(self):
        t = SpellInfo()
        self._check(self.L.rala_hip_get_spell_info(self.h, ctypes.byref(t)))
        return t.as_dict()

    def sequence_slice_info(self):
        t = SequenceSliceInfo()
        self._check(self.L.rala_hip_get_sequence_slice_info(self.h, ctypes.byref(t)))
        return t.as_dict()

    def gzip_timings(self):
        t = GzipTimings()
        self._check(self.L.rala_hip_get_gzip_timings(self.h, ctypes.byref(t)))
        return t.as_dict()

    def gzip_pieces_info(self):
        t = GzipPiecesInfo()
        self._check(self.L.rala_hip_get_gzip_pieces_info(self.h, ctypes.byref(t)))
        return t.as_dict()

    def gzip_member_pieces_info(self):
        t = GzipMemberPiecesInfo()
        self._check(self.L.rala_hip_get_gzip_member_pieces_info(self.h, ctypes.byref(t)))
        return t.as_dict()

    def gzip_members(self):
        """rala_hip_get_gzip_members: (text_off, text_n, crc32) of every member of the gzip file the last ingest inflated"""
        n = ctypes.c_uint64(0)
        self._check(self.L.rala_hip_get_gzip_members(self.h, ctypes.byref(n), 0, None, None, None))
        off, size, crc = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint32)
        self._check(self.L.rala_hip_get_gzip_members(self.h, ctypes.byref(n), n.value, off.ctypes.data, size.ctypes.data, crc.ctypes.data))
        return [(int(a), int(b), int(c)) for a, b, c in zip(off, size, crc)]

    def gzip_find_members(self, data):
        """rala_hip_gzip_find_members: [(header offset, deflate offset)] of every member header among the bytes, found on the device"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        n = ctypes.c_uint64(0)
        self._check(self.L.rala_hip_gzip_find_members(self.h, buf.ctypes.data, len(buf), 0, ctypes.byref(n), None, None))
        head, deflate = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        self._check(self.L.rala_hip_gzip_find_members(self.h, buf.ctypes.data, len(buf), n.value, ctypes.byref(n), head.ctypes.data, deflate.ctypes.data))
        return list(zip(head.tolist(), deflate.tolist()))

    def sequence_timings(self):
        t = IngestTimings()
        self._check(self.L.rala_hip_get_sequence_timings(self.h, ctypes.byref(t)))
        return t.as_dict()

    def set_overlaps(self, ov, later=False):
        """later: RALA_HIP_MEM_HOST_ASYNC - the columns (page-locked, valid until initialize() has returned) are uploaded by
        initialize(), beside its first kernels"""
        c = _soa(ov)
        self.n_overlaps = len(ov)
        self._keep_columns = ov if later else None
        self._check(self.L.rala_hip_set_overlaps(self.h, ctypes.byref(c), self.n_overlaps, MEM_HOST_ASYNC if later else MEM_HOST))

    def set_overlaps_device(self, ptrs, n):
        """ptrs: dict name -> device pointer (int); the memory must outlive the context's use."""
        c = OverlapsC()
        for name, _ in OverlapsC._fields_:
            setattr(c, name, ptrs[name])
        self.n_overlaps = int(n)
        self._check(self.L.rala_hip_set_overlaps(self.h, ctypes.byref(c), self.n_overlaps, MEM_DEVICE))

    # ---- multi-GPU building blocks ----
    def dedupe(self):
        self._check(self.L.rala_hip_dedupe(self.h))

    def emit_bound_tuples(self, tuples_ptr):
        """device pointer of 4 * n_overlaps 8-byte tuples (read | bound << 32), 16-byte aligned"""
        self._check(self.L.rala_hip_emit_bound_tuples(self.h, tuples_ptr))

    def layout(self, x, y, adj_off, adj, iterations, k, t, dt):
        """force-directed layout steps (rala_hip_layout); x, y float64 arrays updated in place"""
        assert x.dtype == np.float64 and y.dtype == np.float64 and x.flags.c_contiguous and y.flags.c_contiguous
        adj_off = np.ascontiguousarray(adj_off, dtype=np.uint32)
        adj = np.ascontiguousarray(adj, dtype=np.uint32)
        self._check(self.L.rala_hip_layout(self.h, len(x), x.ctypes.data, y.ctypes.data, adj_off.ctypes.data,
                                           adj.ctypes.data if len(adj) else None, iterations, k, t, dt))

    def layout_batch(self, comp_off, x, y, adj_off, adj, k, iterations, t, dt):
        """the layout steps of all components in one call (rala_hip_layout_batch): component c's points are
        x / y[comp_off[c]:comp_off[c + 1]] (float64, updated in place), adj holds component-local indices, k one per component"""
        assert x.dtype == np.float64 and y.dtype == np.float64 and x.flags.c_contiguous and y.flags.c_contiguous
        comp_off = np.ascontiguousarray(comp_off, dtype=np.uint32)
        adj_off = np.ascontiguousarray(adj_off, dtype=np.uint32)
        adj = np.ascontiguousarray(adj, dtype=np.uint32)
        k = np.ascontiguousarray(k, dtype=np.float64)
        n_components = max(len(comp_off) - 1, 0)
        assert len(k) == n_components
        self._check(self.L.rala_hip_layout_batch(self.h, n_components, comp_off.ctypes.data if len(comp_off) else None,
                                                 x.ctypes.data, y.ctypes.data, adj_off.ctypes.data if len(adj_off) else None,
                                                 adj.ctypes.data if len(adj) else None, k.ctypes.data, iterations, t, dt))

    def layout_info(self):
        """the last layout_batch: components and points per path, launches, device milliseconds"""
        info = LayoutInfo()
        self._check(self.L.rala_hip_get_layout_info(self.h, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in LayoutInfo._fields_}

    def emit_bound_tuples_bucketed(self, world, tuples_ptr):
        """tuples grouped by owner rank; returns the bucket sizes"""
        counts = np.zeros(world, dtype=np.uint64)
        self._check(self.L.rala_hip_emit_bound_tuples_bucketed(self.h, world, tuples_ptr, counts.ctypes.data))
        return counts

    def device_state(self):
        st = DeviceState()
        self._check(self.L.rala_hip_get_device_state(self.h, ctypes.byref(st)))
        return st

    def copy_device_state(self, **ptrs):
        """device-to-device copy of the named arrays into caller buffers (pointers)"""
        st = DeviceState()
        for k, v in ptrs.items():
            setattr(st, k, v)
        self._check(self.L.rala_hip_copy_device_state(self.h, ctypes.byref(st)))

    def import_state_device(self, **ptrs):
        """ptrs: begin, end, median, p10, alive, n_pits, n_hills, slot, pool, pool_count, valid"""
        st = DeviceState()
        for k, v in ptrs.items():
            setattr(st, k, v)
        self._check(self.L.rala_hip_import_state_device(self.h, ctypes.byref(st)))

    def set_bound_tuples_device(self, tuples_ptr, n):
        self.n_overlaps = 0
        self._check(self.L.rala_hip_set_bound_tuples(self.h, tuples_ptr, int(n), MEM_DEVICE))

    def set_bound_tuples(self, reads, bounds):
        """host arrays (local read, bound) -> packed 8-byte tuples"""
        t = np.ascontiguousarray(reads, dtype=np.uint64) | (np.ascontiguousarray(bounds, dtype=np.uint64) << np.uint64(32))
        self.n_overlaps = 0
        self._check(self.L.rala_hip_set_bound_tuples(self.h, t.ctypes.data, len(t), MEM_HOST))

    def import_state(self, valid, piles, pits, hills):
        """piles: dict as returned by piles(); pits / hills: (offsets, pairs, aux) as intervals()."""
        c = np.ascontiguousarray
        valid = c(valid, dtype=np.uint8)
        arrs = [valid, c(piles["begin"], dtype=np.uint32), c(piles["end"], dtype=np.uint32),
                c(piles["median"], dtype=np.uint16), c(piles["p10"], dtype=np.uint16),
                c(piles["alive"], dtype=np.uint8), c(pits[0], dtype=np.uint64),
                c(pits[1], dtype=np.uint32).reshape(-1), c(pits[2], dtype=np.uint32),
                c(hills[0], dtype=np.uint64), c(hills[1], dtype=np.uint32).reshape(-1)]
        ptrs = [a.ctypes.data if a.size else None for a in arrs]
        if ptrs[6] is None or ptrs[9] is None:
            raise ValueError("interval offsets must have n_reads + 1 entries")
        self._check(self.L.rala_hip_import_state(self.h, *ptrs))

    # ---- stages ----
    def initialize(self):
        self._check(self.L.rala_hip_initialize(self.h))

    def construct(self, sens=None):
        if sens is not None and len(sens):
            c = _soa(sens)
            self._check(self.L.rala_hip_construct(self.h, ctypes.byref(c), len(sens)))
        else:
            self._check(self.L.rala_hip_construct(self.h, None, 0))

    def find_repetitive_hills(self, read, begin, end, median, p10, dataset_median):
        self._check(self.L.rala_hip_find_repetitive_hills(self.h, int(read), int(begin), int(end), int(median), int(p10),
                                                          int(dataset_median)))

    def remove_transitive_edges(self):
        n = ctypes.c_uint32(0)
        self._check(self.L.rala_hip_remove_transitive_edges(self.h, ctypes.byref(n)))
        return int(n.value)

    def tr_mark(self, n_nodes, src, dst, length):
        src = np.ascontiguousarray(src, dtype=np.uint32)
        dst = np.ascontiguousarray(dst, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        marks = np.zeros(len(src), dtype=np.uint8)
        n = ctypes.c_uint32(0)
        self._check(self.L.rala_hip_tr_mark(self.h, n_nodes, len(src), src.ctypes.data, dst.ctypes.data,
                                            length.ctypes.data, marks.ctypes.data, ctypes.byref(n)))
        return marks, int(n.value)

    # ---- results ----
    def valid(self):
        out = np.zeros(self.n_overlaps, dtype=np.uint8)
        self._check(self.L.rala_hip_get_valid(self.h, out.ctypes.data))
        return out

    def piles(self):
        n = self.n_reads
        d = dict(begin=np.zeros(n, np.uint32), end=np.zeros(n, np.uint32), median=np.zeros(n, np.uint16),
                 p10=np.zeros(n, np.uint16), alive=np.zeros(n, np.uint8))
        self._check(self.L.rala_hip_get_piles(self.h, d["begin"].ctypes.data, d["end"].ctypes.data,
                                              d["median"].ctypes.data, d["p10"].ctypes.data,
                                              d["alive"].ctypes.data))
        return d

    def pile_data(self, r):
        out = np.zeros(int(self.read_len[r]), dtype=np.uint16)
        self._check(self.L.rala_hip_get_pile_data(self.h, r, out.ctypes.data))
        return out

    def pile_row_digests(self):
        """checksums of every pile row, computed where the rows lie: (fnv, inside, outside), uint64 per read -
        FNV-1a-64 of Pile::data(), the row's sum inside the valid region, the stored values' sum outside it"""
        out = [np.zeros(self.n_reads, dtype=np.uint64) for _ in range(3)]
        self._check(self.L.rala_hip_get_pile_row_digests(self.h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def pile_rows_info(self):
        """(resident_bytes, rows_materialised): the size of the rows' allocation (0 with option pile_rows = 0) and the rows
        rebuilt from their events since initialize()"""
        out = (ctypes.c_uint64 * 2)()
        self._check(self.L.rala_hip_get_pile_rows_info(self.h, ctypes.addressof(out), ctypes.addressof(out) + 8))
        return int(out[0]), int(out[1])

    def intervals(self, kind):
        """(offsets[n+1] uint64, pairs[k,2] uint32, aux[k] uint32)"""
        offs = np.zeros(self.n_reads + 1, dtype=np.uint64)
        self._check(self.L.rala_hip_get_intervals(self.h, kind, offs.ctypes.data, None, None))
        k = int(offs[-1])
        pairs = np.zeros((k, 2), dtype=np.uint32)
        aux = np.zeros(k, dtype=np.uint32)
        if k:
            self._check(self.L.rala_hip_get_intervals(self.h, kind, offs.ctypes.data, pairs.ctypes.data,
                                                      aux.ctypes.data))
        return offs, pairs, aux

    def overlap_list(self, which=0):
        n = ctypes.c_uint64(0)
        self._check(self.L.rala_hip_get_overlaps(self.h, which, ctypes.byref(n), *([None] * 7)))
        m = int(n.value)
        d = dict(src=np.zeros(m, np.uint32), a_begin=np.zeros(m, np.uint32), a_end=np.zeros(m, np.uint32),
                 b_begin=np.zeros(m, np.uint32), b_end=np.zeros(m, np.uint32), length=np.zeros(m, np.uint32),
                 type=np.zeros(m, np.uint8))
        if m:
            self._check(self.L.rala_hip_get_overlaps(self.h, which, ctypes.byref(n), *[
                d[k].ctypes.data for k in ("src", "a_begin", "a_end", "b_begin", "b_end", "length", "type")]))
        return d

    def graph(self):
        nn, ne = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.rala_hip_get_graph_size(self.h, ctypes.byref(nn), ctypes.byref(ne)))
        nn, ne = int(nn.value), int(ne.value)
        d = dict(node_read=np.zeros(nn, np.uint32), src=np.zeros(ne, np.uint32), dst=np.zeros(ne, np.uint32),
                 len=np.zeros(ne, np.uint32), marked=np.zeros(ne, np.uint8))
        self._check(self.L.rala_hip_get_graph(self.h, d["node_read"].ctypes.data, d["src"].ctypes.data,
                                              d["dst"].ctypes.data, d["len"].ctypes.data,
                                              d["marked"].ctypes.data))
        return d

    def timings(self):
        t = Timings()
        self._check(self.L.rala_hip_get_timings(self.h, ctypes.byref(t)))
        return t.as_dict()

    def num_prefiltered(self):
        n = ctypes.c_uint64(0)
        self._check(self.L.rala_hip_get_num_prefiltered(self.h, ctypes.byref(n)))
        return int(n.value)


def slice_cuts(a_id, world, b_id=None):
    """rala_hip_mg_slice_cuts: world + 1 file positions, cuts on a_id-run boundaries (records whose
    query or target is NO_READ do not break a run)"""
    a = np.ascontiguousarray(a_id, dtype=np.uint32)
    b = None if b_id is None else np.ascontiguousarray(b_id, dtype=np.uint32)
    cuts = np.zeros(world + 1, dtype=np.uint64)
    rc = lib().rala_hip_mg_slice_cuts(a.ctypes.data if len(a) else None, b.ctypes.data if b is not None and len(b) else None,
                                      len(a), world, cuts.ctypes.data)
    if rc != 0:
        raise RalaHipError(rc, "slice_cuts")
    return [int(c) for c in cuts]


def unique_id():
    """128-byte RCCL id (rank 0 makes it, the others receive the bytes)"""
    buf = ctypes.create_string_buffer(128)
    rc = lib().rala_hip_mg_unique_id(buf)
    if rc != 0:
        raise RalaHipError(rc, "no usable RCCL")
    return buf.raw


class ShardedRank:
    """One rank of a sharded run (rala_hip_mg_*).  token: 128-byte RCCL id (bytes) or a LocalGroup; token None: only the
    rank's device contexts are created (not collective) and join(token) enters the group later - launchers make sure
    every rank has its contexts before anybody joins."""

    def __init__(self, device, rank, world, token=None):
        self.L = lib()
        self.rank, self.world = rank, world
        h = ctypes.c_void_p()
        rc = self.L.rala_hip_mg_create_contexts(device, rank, world, ctypes.byref(h))
        if rc != 0:
            raise RalaHipError(rc, "rala_hip_mg_create_contexts failed (device %d, rank %d of %d)" % (device, rank, world))
        self.h = h
        self._keep = None
        self._token = None
        if token is not None:
            try:
                self.join(token)
            except Exception:
                self.close()
                raise

    def join(self, token):
        """collective: every rank of the group calls it (ncclCommInitRank / the in-process rendezvous)"""
        if isinstance(token, LocalGroup):
            self._token = token
            rc = self.L.rala_hip_mg_join(self.h, COMM_LOCAL, token.h)
        else:
            self._token = ctypes.create_string_buffer(bytes(token), 128)
            rc = self.L.rala_hip_mg_join(self.h, COMM_RCCL, self._token)
        self._check(rc)

    def close(self):
        if getattr(self, "h", None):
            self.L.rala_hip_mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RalaHipError(rc, self.L.rala_hip_mg_last_error(self.h).decode())

    def set_reads(self, read_len):
        rl = np.ascontiguousarray(read_len, dtype=np.uint32)
        self.read_len = rl
        self._check(self.L.rala_hip_mg_set_reads(self.h, rl.ctypes.data, len(rl)))

    def set_overlaps(self, ov_slice, first):
        c = _soa(ov_slice)
        self.n_slice = len(ov_slice)
        self._check(self.L.rala_hip_mg_set_overlaps(self.h, ctypes.byref(c), len(ov_slice), int(first), MEM_HOST))

    def run(self, sens_slice=None):
        n = ctypes.c_uint32(0)
        if sens_slice is not None:          # an EMPTY share still takes part in the collective sensitive pass
            c = _soa(sens_slice)
            self._check(self.L.rala_hip_mg_run(self.h, ctypes.byref(c), len(sens_slice), ctypes.byref(n)))
        else:
            self._check(self.L.rala_hip_mg_run(self.h, None, 0, ctypes.byref(n)))
        return int(n.value)

    def context(self):
        """the replicated result as a (borrowed) Context: piles(), intervals(), overlap_list(), graph() ..."""
        c = Context(_borrowed=self.L.rala_hip_mg_context(self.h))
        c.read_len = self.read_len
        c.n_reads = len(self.read_len)
        c.n_overlaps = self.n_slice
        return c

    def pile_data(self, r):
        out = np.zeros(int(self.read_len[r]), dtype=np.uint16)
        self._check(self.L.rala_hip_mg_get_pile_data(self.h, int(r), out.ctypes.data))
        return out

    def pile_row_digests(self):
        """(fnv, inside, outside) of the rows this rank owns: entry j = read j * world + rank"""
        n_own = len(range(self.rank, len(self.read_len), self.world))
        out = [np.zeros(n_own, dtype=np.uint64) for _ in range(3)]
        self._check(self.L.rala_hip_mg_get_pile_row_digests(self.h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def owner_timings(self):
        """stage timings of the owner context (bucketing and pile kernels over the owned reads)"""
        c = Context(_borrowed=self.L.rala_hip_mg_owner_context(self.h))
        return c.timings()

    def timings(self):
        t = MgTimings()
        self._check(self.L.rala_hip_mg_get_timings(self.h, ctypes.byref(t)))
        return t.as_dict()

    def set_option(self, key, value):
        """rala_hip_set_option on the rank's slice context (rala_hip_mg_context)"""
        Context(_borrowed=self.L.rala_hip_mg_context(self.h)).set_option(key, value)

    def layout_batch(self, comp_off, x, y, adj_off, adj, k, iterations, t, dt, out=None):
        """this rank's call of the collective rala_hip_mg_layout_batch (every rank of the group makes it, each on a thread of
        its own); out = (x_out, y_out) float64 arrays or None: no download.  Returns the call's code."""
        arrays = _layout_arrays(comp_off, x, y, adj_off, adj, k)
        ox, oy = (None, None) if out is None else (out[0].ctypes.data, out[1].ctypes.data)
        return self.L.rala_hip_mg_layout_batch(self.h, arrays[0], arrays[1], arrays[2], arrays[3], ox, oy, arrays[4], arrays[5],
                                               arrays[6], iterations, t, dt)

    def layout_info(self):
        """the rank's share of its last layout_batch / layout_ranks: point range, fused components, tiles, launches, gathers ..."""
        info = MgLayoutInfo()
        self._check(self.L.rala_hip_mg_get_layout_info(self.h, ctypes.byref(info)))
        return info.as_dict()


class LocalGroup:
    """rendezvous object of ranks that are threads of this process (RALA_HIP_COMM_LOCAL)"""

    def __init__(self, world):
        self.L = lib()
        h = ctypes.c_void_p()
        rc = self.L.rala_hip_mg_local_group_create(world, ctypes.byref(h))
        if rc != 0:
            raise RalaHipError(rc, "local group")
        self.h, self.world = h, world

    def close(self):
        if getattr(self, "h", None):
            self.L.rala_hip_mg_local_group_destroy(self.h)
            self.h = None


def run_ranks(ranks, sens_slices=None):
    """rala_hip_mg_run_threads: all ranks of this process, one host thread each"""
    L = lib()
    n = len(ranks)
    arr = (ctypes.c_void_p * n)(*[r.h for r in ranks])
    pairs = ctypes.c_uint32(0)
    if sens_slices is not None and any(s is None for s in sens_slices):
        # (tests) ranks that disagree on whether there is a sensitive pass: one Python thread per rank
        import threading
        rcs = [0] * n

        def one(k):
            try:
                ranks[k].run(sens_slices[k])
            except RalaHipError as e:
                rcs[k] = e
        th = [threading.Thread(target=one, args=(k,)) for k in range(n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        bad = [e for e in rcs if e != 0]
        if bad:
            raise bad[0]
        return 0
    if sens_slices is not None:
        cs = (OverlapsC * n)(*[_soa(s) for s in sens_slices])
        ns = (ctypes.c_uint64 * n)(*[len(s) for s in sens_slices])
        rc = L.rala_hip_mg_run_threads(arr, n, cs, ns, ctypes.byref(pairs))
    else:
        rc = L.rala_hip_mg_run_threads(arr, n, None, None, ctypes.byref(pairs))
    if rc != 0:
        msgs = [L.rala_hip_mg_last_error(r.h).decode() for r in ranks]
        raise RalaHipError(rc, " | ".join(m for m in msgs if m))
    return int(pairs.value)


def _layout_arrays(comp_off, x, y, adj_off, adj, k):
    """(n_components, comp_off, x, y, adj_off, adj, k, keep) as the layout calls take them; `keep` holds the converted arrays,
    which must outlive the call"""
    assert x.dtype == np.float64 and y.dtype == np.float64 and x.flags.c_contiguous and y.flags.c_contiguous
    comp_off = np.ascontiguousarray(comp_off, dtype=np.uint32)
    adj_off = np.ascontiguousarray(adj_off, dtype=np.uint32)
    adj = np.ascontiguousarray(adj, dtype=np.uint32)
    k = np.ascontiguousarray(k, dtype=np.float64)
    n_components = max(len(comp_off) - 1, 0)
    assert len(k) == n_components
    return (n_components, comp_off.ctypes.data if len(comp_off) else None, x.ctypes.data, y.ctypes.data,
            adj_off.ctypes.data if len(adj_off) else None, adj.ctypes.data if len(adj) else None, k.ctypes.data,
            (comp_off, adj_off, adj, k))


def layout_ranks(ranks, comp_off, x, y, adj_off, adj, k, iterations, t, dt):
    """rala_hip_mg_layout_batch_threads: the layout steps of all components by all ranks of this process together, one host
    thread per rank; x / y (float64) updated in place from rank 0's download"""
    L = lib()
    n = len(ranks)
    arr = (ctypes.c_void_p * n)(*[r.h for r in ranks])
    a = _layout_arrays(comp_off, x, y, adj_off, adj, k)
    rc = L.rala_hip_mg_layout_batch_threads(arr, n, a[0], a[1], a[2], a[3], a[4], a[5], a[6], iterations, t, dt)
    if rc != 0:
        msgs = [L.rala_hip_mg_last_error(r.h).decode() for r in ranks]
        raise RalaHipError(rc, " | ".join(m for m in msgs if m))


def layout_split(comp_off, fused_max, parts, with_cost=True):
    """rala_hip_layout_split (no device): (first_point[parts + 1], cost[parts]) of the split of a batch's points over the parts,
    or None where it is refused"""
    comp_off = np.ascontiguousarray(comp_off, dtype=np.uint32)
    first = np.zeros(parts + 1, dtype=np.uint32)
    cost = np.zeros(max(parts, 1), dtype=np.uint64)
    rc = lib().rala_hip_layout_split(max(len(comp_off) - 1, 0), comp_off.ctypes.data if len(comp_off) else None, fused_max, parts,
                                     first.ctypes.data, cost.ctypes.data if with_cost else None)
    if rc != 0:
        return None
    return [int(v) for v in first], [int(v) for v in cost[:parts]]


def crc32_chain(reg, length):
    """rala_hip_crc32_chain (no device): the CRC32 of pieces laid end to end from every piece's register (from zero, no final
    inversion) and length"""
    reg = np.ascontiguousarray(reg, dtype=np.uint32)
    length = np.ascontiguousarray(length, dtype=np.uint64)
    assert len(reg) == len(length)
    return int(lib().rala_hip_crc32_chain(reg.ctypes.data, length.ctypes.data, len(reg)))


def gzip_chain(starts, end_bit, text, nxt, status, refuted, end, isize):
    """rala_hip_gzip_chain (no device): the chain of true chunks from chunk 0 through what the device found and counted per
    chunk -> (None when refused, else the jobs' start_bit, stop_bit, text_off, text_n), the walk's counters"""
    u64a, u32a = (lambda a: np.ascontiguousarray(a, dtype=np.uint64)), (lambda a: np.ascontiguousarray(a, dtype=np.uint32))
    starts, end_bit, text, nxt, status, refuted = u64a(starts), u64a(end_bit), u64a(text), u32a(nxt), u32a(status), u32a(refuted)
    n = len(starts)
    assert all(len(a) == n for a in (end_bit, text, nxt, status, refuted))
    out = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
    n_jobs, valid, tm = ctypes.c_uint64(0), ctypes.c_int32(0), GzipTimings()
    rc = lib().rala_hip_gzip_chain(starts.ctypes.data, end_bit.ctypes.data, text.ctypes.data, nxt.ctypes.data, status.ctypes.data,
                                   refuted.ctypes.data, n, end, isize, n, ctypes.byref(n_jobs), *[a.ctypes.data for a in out],
                                   ctypes.byref(tm), ctypes.byref(valid))
    assert rc == 0
    return (tuple(a[:n_jobs.value] for a in out) if valid.value else None), tm.as_dict()


def gzip_pieces(job_start_bit, deflate_off, chunk_bytes, n_chunks, parts):
    """rala_hip_gzip_pieces (no device): first_job[parts + 1] of the chain's split over the parts, or None where it is refused"""
    bits = np.ascontiguousarray(job_start_bit, dtype=np.uint64)
    first = np.zeros(parts + 1, dtype=np.uint64)
    rc = lib().rala_hip_gzip_pieces(bits.ctypes.data, len(bits), deflate_off, chunk_bytes, n_chunks, parts, first.ctypes.data)
    return [int(x) for x in first] if rc == 0 else None


def gzip_compose_windows(out_windows, part):
    """rala_hip_gzip_compose_windows (no device): (the window in front of `part`, valid) from the parts' out-windows, an array of
    parts x 32768 symbols"""
    w = np.ascontiguousarray(out_windows, dtype=np.uint16).reshape(-1, GZIP_WINDOW)
    got, valid = np.zeros(GZIP_WINDOW, dtype=np.uint16), ctypes.c_int32(-1)
    rc = lib().rala_hip_gzip_compose_windows(w.ctypes.data, len(w), part, got.ctypes.data, ctypes.byref(valid))
    if rc != 0:
        raise RalaHipError(rc, "rala_hip_gzip_compose_windows")
    return got, valid.value


def gzip_compose_windows_masked(out_windows, reach, part):
    """rala_hip_gzip_compose_windows_masked (no device): (the window in front of `part` masked in front of the member the part begins
    in, the byte in front of the part from the unmasked window or -1, valid).  out_windows: parts x 32768 uint16; reach: per part,
    the text bytes between the first byte of the member its text begins in and its own first byte."""
    w = np.ascontiguousarray(out_windows, dtype=np.uint16).reshape(-1, GZIP_WINDOW)
    r = np.ascontiguousarray(reach, dtype=np.uint64)
    assert len(r) == len(w)
    got = np.zeros(GZIP_WINDOW, dtype=np.uint16)
    before, valid = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib().rala_hip_gzip_compose_windows_masked(w.ctypes.data, len(w), r.ctypes.data, part, got.ctypes.data, ctypes.byref(before), ctypes.byref(valid))
    if rc != 0:
        raise RalaHipError(rc, "rala_hip_gzip_compose_windows_masked")
    return got, before.value, bool(valid.value)


def gzip_members_proof(members, parts, head, tail, local_bad):
    """rala_hip_gzip_members_proof (no device): (valid, first member that fails).  members: [(text_off, text_n, crc32)]; parts:
    [(begin, end)] of the text; head, tail: [(register, length)] per part; local_bad: per part, a member index or None."""
    m_off, m_n = (np.array([m[k] for m in members], dtype=np.uint64) for k in (0, 1))
    m_crc = np.array([m[2] for m in members], dtype=np.uint32)
    a, b = (np.array([p[k] for p in parts], dtype=np.uint64) for k in (0, 1))
    h_reg, t_reg = (np.array([x[0] for x in regs], dtype=np.uint32) for regs in (head, tail))
    h_len, t_len = (np.array([x[1] for x in regs], dtype=np.uint64) for regs in (head, tail))
    bad_here = np.array([0xFFFFFFFFFFFFFFFF if x is None else x for x in local_bad], dtype=np.uint64)
    assert len(a) == len(h_reg) == len(t_reg) == len(bad_here)
    bad, valid = ctypes.c_uint64(0), ctypes.c_int32(0)
    rc = lib().rala_hip_gzip_members_proof(m_off.ctypes.data, m_n.ctypes.data, m_crc.ctypes.data, len(members), a.ctypes.data, b.ctypes.data, h_reg.ctypes.data,
                                           h_len.ctypes.data, t_reg.ctypes.data, t_len.ctypes.data, bad_here.ctypes.data, len(a), ctypes.byref(bad),
                                           ctypes.byref(valid))
    if rc != 0:
        raise RalaHipError(rc, "rala_hip_gzip_members_proof")
    return bool(valid.value), int(bad.value)


def gzip_chain_members(chunks, cands, file_n, last_crc, last_isize):
    """rala_hip_gzip_chain_members (no device): the chain through a gzip file of several members.  chunks: dict of the arrays
    starts, end_bit, text, next, status, refuted; cands: dict of header_off, deflate_bit, prev_crc, prev_isize, end_bit, text, next,
    status (ascending header_off) -> (None when refused, else (jobs: start_bit, stop_bit, text_off, text_n, first; members:
    [(text_off, text_n, crc32)])), the walk's counters"""
    u64a, u32a = (lambda a: np.ascontiguousarray(a, dtype=np.uint64)), (lambda a: np.ascontiguousarray(a, dtype=np.uint32))
    c = [u64a(chunks["starts"]), u64a(chunks["end_bit"]), u64a(chunks["text"]), u32a(chunks["next"]), u32a(chunks["status"]), u32a(chunks["refuted"])]
    k = [u64a(cands["header_off"]), u64a(cands["deflate_bit"]), u32a(cands["prev_crc"]), u32a(cands["prev_isize"]), u64a(cands["end_bit"]),
         u64a(cands["text"]), u32a(cands["next"]), u32a(cands["status"])]
    n, nk = len(c[0]), len(k[0])
    assert all(len(a) == n for a in c) and all(len(a) == nk for a in k)
    cap = n + nk + 1
    jobs = [np.zeros(cap, dtype=np.uint64) for _ in range(4)] + [np.zeros(cap, dtype=np.uint32)]
    mem = [np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)]
    n_jobs, n_members, valid, tm = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int32(0), GzipTimings()
    rc = lib().rala_hip_gzip_chain_members(*[a.ctypes.data for a in c], n, *[a.ctypes.data for a in k], nk, file_n, last_crc, last_isize, cap,
                                           ctypes.byref(n_jobs), *[a.ctypes.data for a in jobs], cap, ctypes.byref(n_members),
                                           *[a.ctypes.data for a in mem], ctypes.byref(tm), ctypes.byref(valid))
    assert rc == 0
    if not valid.value:
        return None, tm.as_dict()
    members = [(int(a), int(b), int(x)) for a, b, x in zip(*[m[:n_members.value] for m in mem])]
    return (tuple(a[:n_jobs.value] for a in jobs), members), tm.as_dict()
