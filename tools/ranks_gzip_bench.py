"""The input stage of `rala --gpus 8` from a `gzip -6` overlap file - one gzip member that is not BGZF -, the host reader against
the ranks taking the file together on the device (RALA_DEVICE_COMPRESSED=1 RALA_DEVICE_GZIP=1; library: options gzip_on_device
and gzip_in_pieces): the figure that would decide the switches' default for such a run.

    python tools/ranks_gzip_bench.py [c3] [ranks] [--rocprof] > profiles/r21_ranks_gzip.txt

The workload's PAF is written with the repository's generator and compressed by `gzip -6`.  The CLI runs with `ranks` ranks (8)
that share device 0 through the in-process transport.  After one untimed pass of each leg, three alternations of the host leg
(switches off - what such a run gets today, and the yardstick; never the single-context figure) and the device leg in one
session.  Timed: the CLI's `[rala::Graph::initialize] loaded overlaps` stage line; the process is ended once it is out.
Printed: one JSON line with the stage times and, per rank of the last device leg, the piece's figures as the library's trace
line gives them (rala_hip_get_gzip_pieces_info: chunks, jobs, halo jobs, text, symbols through the window in front, longest
chase, compose time).  A later change may turn the switches on for such runs when the device leg wins all three alternations.

PROXY CAVEAT: all ranks share ONE device here, so their device work - find, count, write, compose, resolve, tokenise - runs one
rank after the other, and every rank ships the whole compressed file over the same link: the device leg's figure is the SUM of
the ranks' work and pessimistic for it.

--rocprof: one more device leg of its own under rocprofv3 --kernel-trace --stats (nothing else traced), for the line of
gzip_window_compose_kernel beside its neighbours; its output goes to the directory named in the JSON line."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rala_amd import build
from rala_amd.cpus import effective_cpus
from rala_amd.synth import Dataset

STAGE = "[rala::Graph::initialize] loaded overlaps"
PIECE = re.compile(r"\[trace\] device inflate: part (\d+) of (\d+) of one gzip member: chunks \[(\d+), (\d+)\) of (\d+), jobs \[(\d+), (\d+)\) and (\d+) "
                   r"for the halo, text \[(\d+), (\d+)\) of (\d+); (\d+) own symbols through the window in front \(longest chase (\d+) hops\), "
                   r"compose ([0-9.]+) ms; find ([0-9.]+) ms, decode ([0-9.]+) ms, resolve ([0-9.]+) ms, the file shipped in ([0-9.]+) ms")
LIMIT = 900         # seconds for one run of the CLI


def environment(ranks, device):
    env = dict(os.environ, RALA_COMM="local", RALA_GPUS=str(ranks), RALA_GPU_DEVICES=",".join(["0"] * ranks), RALA_HIP_TRACE="1")
    for k in ("RALA_DEVICE_COMPRESSED", "RALA_DEVICE_GZIP", "RALA_DEVICE_INGEST"):
        env.pop(k, None)
    if device:
        env.update(RALA_DEVICE_COMPRESSED="1", RALA_DEVICE_GZIP="1")
    return env


def leg(exe, fa, gz, ranks, device, threads):
    """-> seconds of the stage line, the ranks' pieces (device leg)"""
    p = subprocess.Popen(["timeout", "-k", "10", str(LIMIT), exe, "-t", str(threads), fa, gz], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                         env=environment(ranks, device), text=True)
    seconds, pieces = None, {}
    for line in p.stderr:
        m = PIECE.match(line)
        if m:
            v = m.groups()
            pieces[int(v[0])] = {"own_chunks": int(v[3]) - int(v[2]), "own_jobs": int(v[6]) - int(v[5]), "halo_jobs": int(v[7]),
                                 "own_text_bytes": int(v[9]) - int(v[8]), "window_markers": int(v[11]), "longest_chase": int(v[12]),
                                 "compose_ms": float(v[13]), "find_ms": float(v[14]), "decode_ms": float(v[15]), "resolve_ms": float(v[16]),
                                 "ship_ms": float(v[17])}
        m = re.match(re.escape(STAGE) + r" (\d+\.\d+) s", line)
        if m:
            seconds = float(m.group(1))
            break
    p.terminate()
    p.wait()
    if seconds is None:
        raise RuntimeError("rala ended without its stage line")
    if device and len(pieces) != ranks:
        raise RuntimeError("the device leg did not take the file: %d of %d ranks inflated a piece" % (len(pieces), ranks))
    if not device and pieces:
        raise RuntimeError("the host leg inflated on the device")
    return seconds, [pieces[k] for k in sorted(pieces)]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    wl = args[0] if args else "c3"
    ranks = int(args[1]) if len(args) > 1 else 8
    threads = effective_cpus()
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset.config(wl)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        fa, paf = os.path.join(d, "reads.fasta"), os.path.join(d, "ovl.paf")
        t0 = time.time()
        ds.write_fasta(fa)
        ds.write_paf(paf)
        text_bytes = os.path.getsize(paf)
        with open(paf + ".gz", "wb") as f:
            subprocess.run(["gzip", "-6", "-c", paf], stdout=f, check=True)
        os.remove(paf)
        gz_bytes = os.path.getsize(paf + ".gz")
        print("[ranks_gzip] %s: %.2f GB of PAF as %.2f GB by gzip -6 in %.1f s" % (wl, text_bytes / 1e9, gz_bytes / 1e9, time.time() - t0), file=sys.stderr)
        leg(exe, fa, paf + ".gz", ranks, False, threads)            # (untimed: the file into the page cache, the device warm)
        leg(exe, fa, paf + ".gz", ranks, True, threads)
        rounds, pieces = [], []
        for _ in range(3):
            host, _ = leg(exe, fa, paf + ".gz", ranks, False, threads)
            device, pieces = leg(exe, fa, paf + ".gz", ranks, True, threads)
            rounds.append({"host_s": host, "device_s": device})
        trace_dir = None
        if "--rocprof" in sys.argv:
            trace_dir = os.path.join(os.getcwd(), "ranks_gzip_rocprof")
            subprocess.run(["timeout", "-k", "10", str(LIMIT), "rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "--", exe, "-t", str(threads),
                            fa, paf + ".gz"], stdout=subprocess.DEVNULL, env=environment(ranks, True), check=True)
    n = len(ds.overlaps.a_id)
    print(json.dumps({
        "workload": wl, "ranks_on_one_device": ranks, "overlaps": n, "text_bytes": text_bytes, "gzip_bytes": gz_bytes, "alternations": rounds,
        "device_wins_all": all(r["device_s"] < r["host_s"] for r in rounds),
        "host_overlaps_per_s": [n / r["host_s"] for r in rounds], "device_overlaps_per_s": [n / r["device_s"] for r in rounds],
        "pieces_of_the_last_device_leg": pieces, "kernel_trace": trace_dir,
        "caveat": "the ranks share one device: their device work serialises and every rank ships the whole file over the same link; the device "
                  "leg is the sum of the ranks' work and pessimistic",
    }))


if __name__ == "__main__":
    main()
