"""Node bases as spans against node bases as strings: `rala -u` on the generator's data with RALA_DEVICE_CONTIGS off (what such a
run gets today: the yardstick) and on, each setting in a process of its own.

  files     the reads as plain FASTA, and as `gzip -6` FASTQ read through the device's index (RALA_DEVICE_SEQUENCES=1
            RALA_DEVICE_GZIP=1 on both legs: with the switch on the slice then keeps its bases on the device)
  schedule  one untimed pass of each leg, then the legs alternate three times
  per run   the stage lines "[rala::Graph::construct] loaded sequences" and "[rala::Graph::simplify]", the wall time from
            the simplify line to the process' exit (unitigs, spelling or string concatenation, printing), the peak resident
            set (ru_maxrss of wait4: the process' VmHWM), and with the switch on the trace line of rala_hip_spell - spans,
            bytes, windows, upload / kernel / copy milliseconds - and the kernel's bytes (one read and one written per
            output byte) over its time as a fraction of 6.3 TB/s

  python tools/spell_bench.py [--config c2 c3] [--dir DIR] [--keep]

--keep leaves the files in DIR (for a profiler's run of one leg: rocprofv3 --kernel-trace --stats -- rala -u reads.fasta ovl.paf).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rala_amd import build  # noqa: E402
from rala_amd.synth import Dataset  # noqa: E402

PEAK_BYTES_PER_S = 6.3e12


def run(exe, reads, paf, env):
    """one `rala -u`: the stage lines' seconds, the tail's wall time, the peak resident set, the spell trace"""
    p = subprocess.Popen([exe, "-u", reads, paf], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
    out = {"loaded_sequences_s": None, "simplify_s": None, "spell": None, "path": None}
    t_simplify = None
    for raw in p.stderr:
        line = raw.decode(errors="replace").rstrip("\n")
        m = re.match(r"\[rala::Graph::construct\] loaded sequences ([0-9.]+) s", line)
        if m:
            out["loaded_sequences_s"] = float(m.group(1))
        m = re.match(r"\[rala::Graph::simplify\] ([0-9.]+) s", line)
        if m:
            out["simplify_s"] = float(m.group(1))
            t_simplify = time.perf_counter()
        if "node bases on the" in line:
            out["path"] = line.split("node bases on the ")[1]
        m = re.search(r"device spell: (\d+) spans, (\d+) bytes in (\d+) windows, upload ([0-9.]+) ms, kernel ([0-9.]+) ms, bytes to the host ([0-9.]+) ms", line)
        if m:
            out["spell"] = dict(zip(("spans", "bytes", "windows"), map(int, m.groups()[:3])))
            out["spell"].update(zip(("upload_ms", "kernel_ms", "copy_ms"), map(float, m.groups()[3:])))
    _, status, usage = os.wait4(p.pid, 0)
    t_end = time.perf_counter()
    p.returncode = os.waitstatus_to_exitcode(status)
    if p.returncode != 0 or t_simplify is None:
        raise RuntimeError("rala failed (%d) on %s" % (p.returncode, reads))
    out["tail_s"] = t_end - t_simplify
    out["peak_rss_mb"] = usage.ru_maxrss / 1024.0
    return out


def show(tag, r):
    print("    %-3s loaded sequences %7.3f s  simplify %7.3f s  simplify -> exit %7.3f s  peak RSS %8.0f MB%s"
          % (tag, r["loaded_sequences_s"], r["simplify_s"], r["tail_s"], r["peak_rss_mb"], "  (%s)" % r["path"] if r["path"] else ""), flush=True)
    if r["spell"]:
        s = r["spell"]
        rate = 2.0 * s["bytes"] / (s["kernel_ms"] * 1e-3) if s["kernel_ms"] > 0 else 0.0
        print("        rala_hip_spell: %d spans, %d bytes, %d windows; upload %.2f ms, kernel %.2f ms, copy %.2f ms; kernel %.1f GB/s = %.1f %% of 6.3 TB/s"
              % (s["spans"], s["bytes"], s["windows"], s["upload_ms"], s["kernel_ms"], s["copy_ms"], rate / 1e9, 100.0 * rate / PEAK_BYTES_PER_S), flush=True)


def legs(exe, what, reads, paf, base_env):
    off = dict(base_env, RALA_HIP_TRACE="1")
    on = dict(off, RALA_DEVICE_CONTIGS="1")
    print("  %s" % what, flush=True)
    run(exe, reads, paf, off)
    run(exe, reads, paf, on)
    wins = []
    for k in range(3):
        a = run(exe, reads, paf, off)
        show("off", a)
        b = run(exe, reads, paf, on)
        show("on", b)
        total = lambda r: r["loaded_sequences_s"] + r["tail_s"]     # noqa: E731  (the two places the switch changes)
        wins.append((total(a), total(b)))
    print("    loaded sequences + simplify -> exit, off / on: %s; the device leg won %d of 3"
          % (", ".join("%.3f / %.3f s" % w for w in wins), sum(1 for a, b in wins if b < a)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["c2"])
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    build.build_host()
    exe = os.path.join(ROOT, "rala_amd", "host", "rala")
    work = tempfile.mkdtemp(dir=args.dir)
    try:
        for name in args.config:
            ds = Dataset.config(name)
            fa, paf, fq = (os.path.join(work, "%s.%s" % (name, ext)) for ext in ("fasta", "paf", "fastq"))
            ds.write_fasta(fa)
            ds.write_paf(paf)
            with open(fa, "rb") as src, open(fq, "wb") as dst:
                while True:
                    head, seq = src.readline(), src.readline()
                    if not head:
                        break
                    dst.write(b"@" + head[1:] + seq + b"+\n" + b"I" * (len(seq) - 1) + b"\n")
            subprocess.check_call(["gzip", "-6", "-f", fq])
            print("%s: %d reads, %.2f GB of FASTA" % (name, ds.n_reads, os.path.getsize(fa) / 1e9), flush=True)
            legs(exe, "plain FASTA (host reader)", fa, paf, dict(os.environ))
            legs(exe, "gzip -6 FASTQ (device index and slice)", fq + ".gz", paf, dict(os.environ, RALA_DEVICE_SEQUENCES="1", RALA_DEVICE_GZIP="1"))
            if not args.keep:
                for path in (fa, paf, fq + ".gz"):
                    os.unlink(path)
    finally:
        if not args.keep:
            try:
                os.rmdir(work)
            except OSError:
                pass


if __name__ == "__main__":
    main()
