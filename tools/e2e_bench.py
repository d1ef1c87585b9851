"""End-to-end overlaps/s from PAF text (second figure): multi-threaded
ingest + upload + the whole device path.  python tools/e2e_bench.py [c2|c3] [threads]
RALA_E2E_GZIP=1: the same from a gzip-compressed file (gzip -1; one thread inflates, the others parse);
RALA_E2E_GZIP=bgzf: from a BGZF file (what bgzip writes: members of at most 64 KB), two legs on the same file alternating
three times each - the device leg (the compressed bytes shipped, the members inflated and the text tokenised on the GPU;
ship / inflate / tokenise from the ingest's trace) and the host leg (device_ingest = 0: the host's BGZF reader);
RALA_E2E_GZIP=gzip: the same two legs on one `gzip -6` file of a single member - the device leg with RALA_DEVICE_GZIP=1
(speculative decoding on the GPU), the host leg the streamed reader (one thread inflates).  RALA_E2E_GZIP_CHUNK=bytes: the
device leg's gzip_chunk_bytes (rala_e2e_from_paf_with sets the option); RALA_E2E_GZIP_SWEEP=a,b,c: one device leg at each
of those chunk sizes first, the alternations at the fastest."""
import ctypes
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rala_amd import build
from rala_amd.synth import Dataset

wl = sys.argv[1] if len(sys.argv) > 1 else "c2"
from rala_amd.cpus import effective_cpus
threads = int(sys.argv[2]) if len(sys.argv) > 2 else effective_cpus()
build.build_host()
L = ctypes.CDLL(os.path.join(build.PKG, "host", "librala.so"))
L.rala_e2e_from_paf.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 5
ds = Dataset.config(wl)
with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
    paf = os.path.join(d, "ovl.paf")
    t0 = time.time()
    ds.write_paf(paf)
    size = os.path.getsize(paf)
    print("[e2e] wrote %s: %.2f GB in %.1f s" % (wl, size / 1e9, time.time() - t0), file=sys.stderr)
    if os.environ.get("RALA_E2E_GZIP") == "1":
        import subprocess
        t0 = time.time()
        subprocess.run(["gzip", "-1", paf], check=True)
        paf += ".gz"
        print("[e2e] gzip -1: %.2f GB in %.1f s" % (os.path.getsize(paf) / 1e9, time.time() - t0), file=sys.stderr)
    elif os.environ.get("RALA_E2E_GZIP") == "bgzf":
        # what bgzip writes: gzip members of 64 KB with their size in a "BC" extra field (inflated by several threads)
        import struct
        import zlib
        from concurrent.futures import ThreadPoolExecutor

        def member(data):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            body = c.compress(data) + c.flush()
            return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" +
                    struct.pack("<HH", 2, 18 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))

        t0 = time.time()
        with open(paf, "rb") as src, open(paf + ".gz", "wb") as dst, ThreadPoolExecutor(threads) as pool:
            while True:
                chunks = [c for c in (src.read(65280) for _ in range(4096)) if c]
                if not chunks:
                    break
                for m in pool.map(member, chunks):
                    dst.write(m)
            dst.write(member(b""))
        os.remove(paf)
        paf += ".gz"
        print("[e2e] bgzf: %.2f GB in %.1f s" % (os.path.getsize(paf) / 1e9, time.time() - t0), file=sys.stderr)
    elif os.environ.get("RALA_E2E_GZIP") == "gzip":
        import subprocess
        t0 = time.time()
        subprocess.run(["gzip", "-6", paf], check=True)
        paf += ".gz"
        print("[e2e] gzip -6: %.2f GB in %.1f s" % (os.path.getsize(paf) / 1e9, time.time() - t0), file=sys.stderr)
    mode = os.environ.get("RALA_E2E_GZIP")
    if mode in ("bgzf", "gzip"):
        L.rala_e2e_from_paf_with.argtypes = ([ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int] +
                                             [ctypes.c_void_p] * 6)
        read_len = np.ascontiguousarray(ds.read_len, dtype=np.uint32)
        trace_path = os.path.join(d, "trace.txt")

        def leg(device):
            ms = [ctypes.c_double() for _ in range(3)]
            n_ovl, n_tr, used = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_int(-1)
            # (the ingest's trace lines go to stderr: caught in a file for the ship / inflate / tokenise times)
            os.environ["RALA_HIP_TRACE"] = "1"
            if mode == "gzip":
                os.environ["RALA_DEVICE_GZIP"] = "1" if device else "0"
            sys.stderr.flush()
            saved = os.dup(2)
            with open(trace_path, "w") as tf:
                os.dup2(tf.fileno(), 2)
                try:
                    rc = L.rala_e2e_from_paf_with(paf.encode(), read_len.ctypes.data, ds.n_reads, threads, device,
                                                  *[ctypes.byref(x) for x in ms], ctypes.byref(n_ovl), ctypes.byref(n_tr), ctypes.byref(used))
                finally:
                    os.dup2(saved, 2)
                    os.close(saved)
                    os.environ.pop("RALA_HIP_TRACE", None)
            trace = [x for x in open(trace_path).read().splitlines() if "device ingest" in x or "device inflate" in x]
            assert rc == 0, rc
            assert used.value == device, (device, used.value)
            tot = sum(x.value for x in ms)
            out = {"device_ingest": device, "ms_parse": ms[0].value, "ms_upload": ms[1].value, "ms_device_first_call": ms[2].value,
                   "ms_total": tot, "overlaps_per_s": n_ovl.value / (tot * 1e-3), "n_overlaps": n_ovl.value, "transitive_pairs": n_tr.value}
            if device and mode == "gzip":
                ing = [x for x in trace if "device ingest" in x][-1]
                inf = [x for x in trace if "device inflate" in x][-1]
                out["ms_ship_compressed"] = float(inf.split(" shipped in ")[1].split(" ms")[0])
                out["ms_tokenise"] = float(ing.split(" tokenised in ")[1].split(" ms")[0])
                for k in ("find", "decode", "resolve"):
                    out["ms_" + k] = float(inf.split(" %s " % k)[1].split(" ms")[0])
                for k in ("chunks", "with a candidate", "confirmed", "refuted"):
                    out["chunks" if k == "chunks" else "chunks_" + k.replace(" ", "_")] = int(inf.split(" " + k)[0].split()[-1].lstrip("("))
                out["trace"] = trace
            elif device:
                ing = [x for x in trace if "device ingest" in x][-1]
                inf = [x for x in trace if "device inflate" in x][-1]
                out["ms_ship_compressed"] = float(ing.split(" shipped in ")[1].split(" ms")[0]) + float(inf.split("(index and ship ")[1].split(" ms")[0])
                out["ms_tokenise"] = float(ing.split(" tokenised in ")[1].split(" ms")[0])
                out["ms_inflate"] = float(inf.split(" inflated in ")[1].split(" ms")[0])
                out["trace"] = trace
            print("[e2e] %s leg: parse %.1f ms, upload %.1f ms, device %.1f ms, total %.1f ms = %.1f M overlaps/s" % (
                "device" if device else "host", ms[0].value, ms[1].value, ms[2].value, tot, out["overlaps_per_s"] / 1e6), file=sys.stderr)
            return out

        sweep = []
        if mode == "gzip" and os.environ.get("RALA_E2E_GZIP_SWEEP"):
            # device legs at each gzip_chunk_bytes of the list; the alternations then run at the fastest one
            for chunk in os.environ["RALA_E2E_GZIP_SWEEP"].split(","):
                os.environ["RALA_E2E_GZIP_CHUNK"] = chunk
                r = leg(1)
                sweep.append({"gzip_chunk_bytes": int(chunk), **{k: r[k] for k in r if k.startswith("ms_") or k.startswith("chunks")}})
            os.environ["RALA_E2E_GZIP_CHUNK"] = str(min(sweep, key=lambda x: x["ms_total"])["gzip_chunk_bytes"])
        runs = []
        for rep in range(3):
            runs.append((leg(1), leg(0)))
        dev = min((r[0] for r in runs), key=lambda x: x["ms_total"])
        host = min((r[1] for r in runs), key=lambda x: x["ms_total"])
        assert all(r[0]["transitive_pairs"] == r[1]["transitive_pairs"] == dev["transitive_pairs"] for r in runs)
        assert all(r[0]["n_overlaps"] == r[1]["n_overlaps"] for r in runs)
        print(json.dumps({"workload": wl, "paf_bytes": size, "bgzf_bytes" if mode == "bgzf" else "gzip_bytes": os.path.getsize(paf), "threads": threads,
                          "n_overlaps": dev["n_overlaps"], "transitive_pairs": dev["transitive_pairs"], "device": dev, "host": host,
                          "alternations": [{"device_ms_total": a["ms_total"], "host_ms_total": b["ms_total"],
                                            "host_over_device": b["ms_total"] / a["ms_total"]} for a, b in runs],
                          "min_host_over_device": min(b["ms_total"] / a["ms_total"] for a, b in runs),
                          **({"gzip_chunk_bytes": os.environ.get("RALA_E2E_GZIP_CHUNK", "default"), "sweep": sweep} if mode == "gzip" else {})}))
        sys.exit(0)
    best = None
    # RALA_E2E_AB=VAR: alternate runs without and with the environment variable VAR=1 (reader variants), report both
    ab = os.environ.get("RALA_E2E_AB")
    for rep in range(8 if ab else 3):
        if ab:
            if rep & 1:
                os.environ[ab] = "1"
            else:
                os.environ.pop(ab, None)
        ms = [ctypes.c_double() for _ in range(3)]
        n_ovl, n_tr = ctypes.c_uint64(), ctypes.c_uint32()
        read_len = np.ascontiguousarray(ds.read_len, dtype=np.uint32)
        rc = L.rala_e2e_from_paf(paf.encode(), read_len.ctypes.data, ds.n_reads, threads, *[ctypes.byref(x) for x in ms],
                                 ctypes.byref(n_ovl), ctypes.byref(n_tr))
        assert rc == 0, rc
        tot = sum(x.value for x in ms)
        if ab:
            print("[e2e] %s=%d: parse %.1f ms, upload %.1f ms, device %.1f ms, total %.1f ms = %.1f M overlaps/s" % (
                ab, rep & 1, ms[0].value, ms[1].value, ms[2].value, tot, n_ovl.value / tot / 1e3), file=sys.stderr)
        if best is None or tot < best["ms_total"]:
            best = {"workload": wl, "paf_bytes": size, "n_overlaps": n_ovl.value, "threads": threads,
                    "ms_parse": ms[0].value, "ms_upload": ms[1].value, "ms_device_first_call": ms[2].value, "ms_total": tot,
                    "overlaps_per_s": n_ovl.value / (tot * 1e-3), "parse_GB_per_s": size / 1e9 / (ms[0].value * 1e-3),
                    "transitive_pairs": n_tr.value}
print(json.dumps(best))
