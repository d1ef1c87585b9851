"""A read file that is one `gzip -6` member, host reader against device path: the CLI's two "loaded sequences" stage lines.

    python tools/sequence_gzip_bench.py [--reads N] [--alternations K] [--out profiles/r12_sequence_gzip.txt] [--rocprof]

Generates a FASTQ with the repository's generator (default 100 000 reads of about 10 kb: 1 Gbase), compresses it with `gzip -6`,
then alternates the host leg (RALA_DEVICE_SEQUENCES=0 RALA_DEVICE_GZIP=0: what the CLI does by default) and the device leg (both
1) K times in the same build.  Every step that uses the GPU runs under its own time limit, and the script stops at the first one
that fails.  The result file holds both legs' times, the trace lines of the device leg (rala_hip_get_gzip_timings,
rala_hip_get_sequence_timings, rala_hip_get_sequence_slice_info as the library prints them) and the gather kernel's rate in GB/s
of text against the 6.3 TB/s an MI355X streams."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.3


def stage_times(err):
    return [float(x) for x in re.findall(r"loaded sequences (\d+\.\d+) s", err)]


def leg(exe, args, switch, limit, prefix=()):
    env = dict(os.environ, RALA_DEVICE_SEQUENCES=switch, RALA_DEVICE_GZIP=switch, RALA_HIP_TRACE="1")
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode()[-4000:])
        raise SystemExit("the %s leg ended with %d: stopping" % ("device" if switch == "1" else "host", r.returncode))
    return time.time() - t0, r.stdout, r.stderr.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds one leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_sequence_gzip.txt"))
    ap.add_argument("--rocprof", action="store_true", help="one more device leg under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    from rala_amd import build
    from rala_amd.synth import Dataset
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as d:
        ds = Dataset(a.reads, 200 * a.reads, 3)
        fa, paf, fq = os.path.join(d, "reads.fasta"), os.path.join(d, "ovl.paf"), os.path.join(d, "reads.fastq")
        ds.write_fasta(fa)
        ds.write_paf(paf)
        with open(fa, "rb") as f, open(fq, "wb") as out:
            while True:
                name, seq = f.readline().rstrip(b"\n"), f.readline().rstrip(b"\n")
                if not name:
                    break
                out.write(b"@" + name[1:] + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
        os.remove(fa)
        text_bytes = os.path.getsize(fq)
        t0 = time.time()
        subprocess.check_call(["gzip", "-6", fq])
        gz = fq + ".gz"
        say("%d reads, %.3f Gbase, %.3f GB of FASTQ text, %.3f GB as one gzip -6 member (compressed in %.0f s)" % (
            ds.n_reads, int(ds.read_len.sum()) / 1e9, text_bytes / 1e9, os.path.getsize(gz) / 1e9, time.time() - t0))
        outs = {}
        for k in range(a.alternations):
            for switch in ("0", "1"):
                wall, out, err = leg(exe, [gz, paf], switch, a.limit)
                st = stage_times(err)
                outs.setdefault(switch, out)
                if out != outs["0"]:
                    raise SystemExit("the legs' outputs differ: stopping")
                say("alternation %d %s leg: loaded sequences %s s (sum %.3f s), wall %.1f s" % (
                    k, "device" if switch == "1" else "host  ", " + ".join("%.3f" % x for x in st), sum(st), wall))
                if switch == "1":
                    for l in err.splitlines():
                        if l.startswith("[trace] device inflate: one gzip member") or l.startswith("[trace] device sequence"):
                            say("    " + l)
                    m = re.search(r"device sequence slice: .*gather (\d+\.\d+) ms", err)
                    if m and float(m.group(1)) > 0:
                        rate = text_bytes / 1e9 / (float(m.group(1)) / 1e3)
                        # (the whole text over the gather kernel's time: a window without a kept read is not gathered, so where
                        # the graph drops reads in runs as long as a window this overstates the rate)
                        say("    gather kernel: %.1f GB/s of text (all of the file's text / gather ms; windows without a kept read are "
                            "not gathered), %.2f %% of %.1f TB/s" % (rate, rate / (STREAM_TBS * 1e3) * 100, STREAM_TBS))
        if a.rocprof:
            with tempfile.TemporaryDirectory() as pd:
                leg(exe, [gz, paf], "1", a.limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", pd, "-o", "seqgz", "--"))
                for base, _, files in os.walk(pd):
                    for f in files:
                        if f.endswith("kernel_stats.csv"):
                            say("rocprofv3 --kernel-trace --stats, device leg:")
                            lines.extend(open(os.path.join(base, f)).read().splitlines()[:25])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
