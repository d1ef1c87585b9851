"""The name table between the device's sequence index and the first tokeniser launch: the host's way against the device's, in
one process, on FASTA files of N reads of 200 bases with 36-byte names (the length of a nanopore read id).

  host leg    what the code does without RALA_DEVICE_NAMES: rala_hip_get_sequence_index (names, offsets, lengths), one string per
              read into an unordered_map, NameTable::build, rala_hip_set_name_table - through the shim of rala_amd/host/io_capi.cpp
  device leg  rala_hip_build_name_table and the same download of the names (they are kept for the graph's nodes)

After one untimed pass of each the two legs alternate three times.  Then `rala` itself on the file with both settings of the
switch: its "[rala::Graph::initialize] loaded sequences" and "loaded overlaps" stage lines (the host's NameTable::build lies in the
second, the device's build in the first).

  python tools/name_table_bench.py [--reads 1000000 4000000] [--dir DIR] [--device-only]
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rala_amd import build, hip  # noqa: E402

ALPHABET = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)


def write_fasta(path, n, seed):
    """n records '>' + 36-byte name (a UUID's shape) + 200 bases, one line each"""
    rng = np.random.default_rng(seed)
    rec = np.empty((n, 1 + 36 + 1 + 200 + 1), dtype=np.uint8)
    rec[:, 0] = ord(">")
    rec[:, 1:37] = ALPHABET[rng.integers(0, 16, size=(n, 36))]
    for k in (9, 14, 19, 24):
        rec[:, k] = ord("-")
    rec[:, 37] = rec[:, -1] = ord("\n")
    rec[:, 38:238] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 200))]
    rec.tofile(path)


def shim():
    build.build_host()
    L = ctypes.CDLL(os.path.join(ROOT, "rala_amd", "host", "libassembly_graph.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.io_names_strings_map_build.restype = vp
    L.io_names_strings_map_build.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.io_names_bucket_ptr.restype = vp
    L.io_names_bucket_ptr.argtypes = [vp]
    L.io_names_arena_ptr.restype = vp
    L.io_names_arena_ptr.argtypes = [vp]
    L.io_names_buckets.restype = u64
    L.io_names_buckets.argtypes = [vp]
    L.io_names_arena_bytes.restype = u64
    L.io_names_arena_bytes.argtypes = [vp]
    L.io_names_free.argtypes = [vp]
    return L


def legs(path, n, device_only):
    S = shim()
    ctx = hip.Context(0)
    L = ctx.L
    nr, nb, irr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    ctx._check(L.rala_hip_index_sequences(ctx.h, os.fsencode(path), 0, 8, ctypes.byref(nr), ctypes.byref(nb), ctypes.byref(irr)))
    assert irr.value == 0 and nr.value == n
    name_off, name_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    arena = np.zeros(nb.value + 1, dtype=np.uint8)

    def download():
        ctx._check(L.rala_hip_get_sequence_index(ctx.h, name_off.ctypes.data, name_len.ctypes.data, None, None, None, arena.ctypes.data))

    def host_leg():
        t0 = time.perf_counter()
        download()
        distinct = ctypes.c_uint64(0)
        t = S.io_names_strings_map_build(arena.ctypes.data, name_off.ctypes.data, name_len.ctypes.data, n, ctypes.byref(distinct))
        ctx._check(L.rala_hip_set_name_table(ctx.h, S.io_names_bucket_ptr(t), S.io_names_buckets(t), S.io_names_arena_ptr(t),
                                             S.io_names_arena_bytes(t)))
        dt = time.perf_counter() - t0
        S.io_names_free(t)
        return dt, distinct.value

    def device_leg():
        t0 = time.perf_counter()
        n_buckets, distinct = ctx.build_name_table()
        download()
        return time.perf_counter() - t0, distinct

    if device_only:
        for _ in range(3):
            device_leg()
        print("device leg alone, %d reads: %s" % (n, ctx.name_table_info()), flush=True)
        ctx.close()
        return
    host_leg()
    device_leg()
    host, device = [], []
    for _ in range(3):
        dt, dh = host_leg()
        host.append(dt)
        dt, dd = device_leg()
        device.append(dt)
        assert dh == dd, (dh, dd)
    info = ctx.name_table_info()
    print("%d reads, %d distinct names, %d bytes of names" % (n, dd, nb.value))
    print("  host leg   (index download, strings + unordered_map, NameTable::build, rala_hip_set_name_table): %s s"
          % ", ".join("%.3f" % x for x in host))
    print("  device leg (rala_hip_build_name_table, index download):                                        %s s"
          % ", ".join("%.4f" % x for x in device))
    print("  rala_hip_get_name_table_info: device_ms %.3f, names %d, distinct %d, n_buckets %d, longest_probe %d"
          % (info["device_ms"], info["names"], info["distinct"], info["n_buckets"], info["longest_probe"]), flush=True)
    ctx.close()


def cli_stage_lines(path, work):
    """rala on the file with an overlap file of one record: the run ends behind the stage lines wanted here ("filtered all
    sequences"); each setting in a process of its own"""
    exe = os.path.join(ROOT, "rala_amd", "host", "rala")
    paf = os.path.join(work, "one.paf")
    with open(path, "rb") as f:
        a = f.readline()[1:].strip().decode()
        f.readline()
        b = f.readline()[1:].strip().decode()
    open(paf, "w").write("%s\t200\t0\t150\t+\t%s\t200\t50\t200\t150\t150\t255\n" % (a, b))
    for names in ("0", "1"):
        env = dict(os.environ, RALA_DEVICE_SEQUENCES="1", RALA_DEVICE_NAMES=names)
        r = subprocess.run([exe, path, paf], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
        for line in r.stderr.decode().splitlines():
            if "loaded sequences" in line or "loaded overlaps" in line:
                print("  rala, RALA_DEVICE_NAMES=%s: %s" % (names, line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--dir", default=None)
    ap.add_argument("--device-only", action="store_true", help="three device legs and nothing else (for a profiler)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=args.dir) as work:
        for n in args.reads:
            path = os.path.join(work, "reads%d.fasta" % n)
            write_fasta(path, n, n)
            legs(path, n, args.device_only)
            if not args.device_only:
                cli_stage_lines(path, work)
            os.unlink(path)


if __name__ == "__main__":
    main()
