"""Overlaps/s end to end from a PAF file that is SEVERAL gzip members (what `cat part*.paf.gz` gives): the path of
tools/e2e_bench.py (rala_e2e_from_paf_with: ingest, upload and the whole device path) on one file, two legs alternating three
times - the device leg (RALA_DEVICE_GZIP=2: member find, chain through the members, every member proven) and the host leg
(device_ingest = 0: the streamed reader, one thread inflates), which is what such a file gets without the option.  The yardstick
is that host leg in the same process, never the single-member device figure.

    python tools/gzip_members_bench.py [c3] [threads] > profiles/r13_gzip_members.txt

The file: the workload's PAF cut into members of 64 MB of text (at line ends or not: wherever the 64 MB end), each `gzip -6`
(zlib level 6).  Printed: one JSON line with both legs' times per alternation, the device leg's trace line (member count, header
candidates, the member find's time) and the false candidates (candidates - members).  The kernel lines come from a run of their
own: rocprofv3 --kernel-trace --stats -- python tools/gzip_members_bench.py c3 (gzip_member_find_kernel, gzip_piece_crc_kernel)."""
import ctypes
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rala_amd import build
from rala_amd.cpus import effective_cpus
from rala_amd.synth import Dataset

MEMBER_TEXT = 64 << 20


def gz_member(text):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else effective_cpus()
    build.build_host()
    L = ctypes.CDLL(os.path.join(build.PKG, "host", "librala.so"))
    L.rala_e2e_from_paf_with.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 6
    ds = Dataset.config(wl)
    read_len = np.ascontiguousarray(ds.read_len, dtype=np.uint32)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        paf = os.path.join(d, "ovl.paf")
        t0 = time.time()
        ds.write_paf(paf)
        size = os.path.getsize(paf)
        print("[members] wrote %s: %.2f GB in %.1f s" % (wl, size / 1e9, time.time() - t0), file=sys.stderr)
        t0 = time.time()
        n_members = 0
        with open(paf, "rb") as src, open(paf + ".gz", "wb") as dst, ThreadPoolExecutor(threads) as pool:
            while True:
                texts = [t for t in (src.read(MEMBER_TEXT) for _ in range(threads)) if t]
                if not texts:
                    break
                for m in pool.map(gz_member, texts):
                    dst.write(m)
                    n_members += 1
        os.remove(paf)
        paf += ".gz"
        print("[members] %d members of %d MB of text at level 6: %.2f GB in %.1f s" % (n_members, MEMBER_TEXT >> 20, os.path.getsize(paf) / 1e9,
                                                                                      time.time() - t0), file=sys.stderr)
        trace_path = os.path.join(d, "trace.txt")

        def leg(device):
            ms = [ctypes.c_double() for _ in range(3)]
            n_ovl, n_tr, used = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_int(-1)
            os.environ["RALA_HIP_TRACE"] = "1"
            os.environ["RALA_DEVICE_GZIP"] = "2" if device else "0"
            sys.stderr.flush()
            saved = os.dup(2)
            with open(trace_path, "w") as tf:
                os.dup2(tf.fileno(), 2)
                try:
                    rc = L.rala_e2e_from_paf_with(paf.encode(), read_len.ctypes.data, ds.n_reads, threads, device, *[ctypes.byref(x) for x in ms],
                                                  ctypes.byref(n_ovl), ctypes.byref(n_tr), ctypes.byref(used))
                finally:
                    os.dup2(saved, 2)
                    os.close(saved)
                    os.environ.pop("RALA_HIP_TRACE", None)
            assert rc == 0, rc
            assert used.value == device, "the %s leg did not run (used_device_ingest %d)" % ("device" if device else "host", used.value)
            tot = sum(x.value for x in ms)
            out = {"device_ingest": device, "ms_parse": ms[0].value, "ms_upload": ms[1].value, "ms_device_first_call": ms[2].value, "ms_total": tot,
                   "overlaps_per_s": n_ovl.value / (tot * 1e-3), "n_overlaps": n_ovl.value, "transitive_pairs": n_tr.value}
            if device:
                inf = [x for x in open(trace_path).read().splitlines() if "device inflate" in x][-1]
                out["trace"] = inf
                out["members"] = int(inf.split(" gzip members")[0].split()[-1]) if " gzip members" in inf else 1
                if " header candidates found in " in inf:
                    out["header_candidates"] = int(inf.split(" header candidates")[0].split("(")[-1])
                    out["false_candidates"] = out["header_candidates"] - out["members"]
                    out["ms_member_find"] = float(inf.split(" header candidates found in ")[1].split(" ms")[0])
            print("[members] %s leg: total %.1f ms = %.1f M overlaps/s" % ("device" if device else "host", tot, out["overlaps_per_s"] / 1e6), file=sys.stderr)
            return out

        runs = [(leg(1), leg(0)) for _ in range(3)]
        assert all(a["transitive_pairs"] == b["transitive_pairs"] and a["n_overlaps"] == b["n_overlaps"] for a, b in runs)
        assert all(a["members"] == n_members for a, _ in runs)
        print(json.dumps({"workload": wl, "paf_bytes": size, "gzip_bytes": os.path.getsize(paf), "members": n_members, "threads": threads,
                          "alternations": [{"device": a, "host": b, "host_over_device": b["ms_total"] / a["ms_total"]} for a, b in runs],
                          "min_host_over_device": min(b["ms_total"] / a["ms_total"] for a, b in runs)}))


if __name__ == "__main__":
    main()
