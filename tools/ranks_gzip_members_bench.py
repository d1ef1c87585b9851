"""The input stages of `rala --gpus 8` from a gzip overlap file of SEVERAL members that is not BGZF - what `cat part*.paf.gz` and
`pigz -i` write - as the primary file and as the -s file: the host reader against the ranks taking the file together on the device
(RALA_DEVICE_COMPRESSED=2 RALA_DEVICE_GZIP=2; library: options gzip_on_device, gzip_in_pieces and gzip_members on every rank,
rala_hip_mg_set_overlaps_from_paf and rala_hip_mg_tokenise_sensitive).  The figures that would decide the switches' default.

    python tools/ranks_gzip_members_bench.py [c3] [ranks] [--members | --sensitive] [--rocprof] > profiles/r23_ranks_gzip_members.txt

The workload's PAF is written with the repository's generator and compressed as members of 64 MB of text each at level 6.  The
CLI runs with `ranks` ranks (8) that share device 0 through the in-process transport.  Per mode: one untimed pass of each leg, then
three alternations of the host leg (switches off - what such a run gets today, and the yardstick; never the single-member device
figure) and the device leg on the same file in one session.
  --members    the file as the primary file; timed: the CLI's `[rala::Graph::initialize] loaded overlaps` stage line
  --sensitive  the same file as the -s file too (`rala -s FILE reads FILE`); timed: the stage line of Graph::construct that holds
               `loaded overlaps` (the -s file read, and the sensitive pass behind it, which is the same work in both legs)
  neither      both modes, one after the other
Printed: one JSON line per mode with the stage times and, per rank of the last device leg, the trace line of its part.  The
device leg has to win all three alternations in both modes before a later change may turn the switches on.

PROXY CAVEAT: all ranks share ONE device here, so their device work runs one rank after the other, and every rank ships the whole
compressed file over the same link: the device leg's figure is the SUM of the ranks' work and pessimistic for it.

--rocprof: one more device leg of its own per mode under rocprofv3 --kernel-trace --stats (nothing else traced), for the lines of
gzip_window_compose_members_kernel and gzip_count_members_kernel beside their neighbours; its output goes to the directory named
in the JSON line."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rala_amd import build
from rala_amd.cpus import effective_cpus
from rala_amd.synth import Dataset

STAGES = {"members": "[rala::Graph::initialize] loaded overlaps", "sensitive": "[rala::Graph::construct] loaded overlaps"}
PART = re.compile(r"\[trace\] device inflate: part (\d+) of (\d+) of (\d+) gzip members")
MEMBER_TEXT = 64 << 20
LIMIT = 1500        # seconds for one run of the CLI


def write_members(paf, dst, member_text=MEMBER_TEXT, level=6):
    """the file's lines as gzip members of about member_text bytes of text each, cut at line starts -> members written"""
    n = 0
    with open(paf, "rb") as src, open(dst, "wb") as out:
        while True:
            text = src.read(member_text)
            if not text:
                break
            text += src.readline()
            c = zlib.compressobj(level, zlib.DEFLATED, 31)
            out.write(c.compress(text) + c.flush())
            n += 1
    return n


def environment(ranks, device):
    env = dict(os.environ, RALA_COMM="local", RALA_GPUS=str(ranks), RALA_GPU_DEVICES=",".join(["0"] * ranks), RALA_HIP_TRACE="1")
    for k in ("RALA_DEVICE_COMPRESSED", "RALA_DEVICE_GZIP", "RALA_DEVICE_INGEST"):
        env.pop(k, None)
    if device:
        env.update(RALA_DEVICE_COMPRESSED="2", RALA_DEVICE_GZIP="2")
    return env


def command(exe, mode, fa, gz, threads):
    return [exe, "-t", str(threads)] + (["-s", gz] if mode == "sensitive" else []) + [fa, gz]


def leg(exe, mode, fa, gz, ranks, device, threads):
    """-> seconds of the mode's stage line, the trace lines of the ranks' parts (device leg)"""
    p = subprocess.Popen(["timeout", "-k", "10", str(LIMIT)] + command(exe, mode, fa, gz, threads), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                         env=environment(ranks, device), text=True)
    seconds, parts = None, []
    for line in p.stderr:
        if PART.match(line):
            parts.append(line.strip())
        m = re.match(re.escape(STAGES[mode]) + r".* (\d+\.\d+) s$", line.rstrip())
        if m:
            seconds = float(m.group(1))
            break
    p.terminate()
    p.wait()
    if seconds is None:
        raise RuntimeError("rala ended without its stage line")
    want = ranks * (2 if mode == "sensitive" else 1)
    if device and len(parts) != want:
        raise RuntimeError("the device leg did not take the file: %d of %d parts inflated" % (len(parts), want))
    if not device and parts:
        raise RuntimeError("the host leg inflated on the device")
    return seconds, parts


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    wl = args[0] if args else "c3"
    ranks = int(args[1]) if len(args) > 1 else 8
    modes = [m for m in ("members", "sensitive") if "--" + m in sys.argv] or ["members", "sensitive"]
    threads = effective_cpus()
    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset.config(wl)
    n = len(ds.overlaps.a_id)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        fa, paf, gz = os.path.join(d, "reads.fasta"), os.path.join(d, "ovl.paf"), os.path.join(d, "members.paf.gz")
        t0 = time.time()
        ds.write_fasta(fa)
        ds.write_paf(paf)
        text_bytes = os.path.getsize(paf)
        n_members = write_members(paf, gz)
        os.remove(paf)
        gz_bytes = os.path.getsize(gz)
        print("[ranks_gzip_members] %s: %.2f GB of PAF as %d members, %.2f GB at level 6, in %.1f s" % (wl, text_bytes / 1e9, n_members, gz_bytes / 1e9,
                                                                                                     time.time() - t0), file=sys.stderr)
        for mode in modes:
            leg(exe, mode, fa, gz, ranks, False, threads)           # (untimed: the file into the page cache, the device warm)
            leg(exe, mode, fa, gz, ranks, True, threads)
            rounds, parts = [], []
            for _ in range(3):
                host, _ = leg(exe, mode, fa, gz, ranks, False, threads)
                device, parts = leg(exe, mode, fa, gz, ranks, True, threads)
                rounds.append({"host_s": host, "device_s": device})
            trace_dir = None
            if "--rocprof" in sys.argv:
                trace_dir = os.path.join(os.getcwd(), "ranks_gzip_members_rocprof_" + mode)
                subprocess.run(["timeout", "-k", "10", str(LIMIT), "rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "--"] +
                               command(exe, mode, fa, gz, threads), stdout=subprocess.DEVNULL, env=environment(ranks, True), check=True)
            print(json.dumps({
                "mode": mode, "stage_line": STAGES[mode], "workload": wl, "ranks_on_one_device": ranks, "overlaps": n, "text_bytes": text_bytes,
                "members": n_members, "member_text_bytes": MEMBER_TEXT, "gzip_bytes": gz_bytes, "alternations": rounds,
                "device_wins_all": all(r["device_s"] < r["host_s"] for r in rounds),
                "host_overlaps_per_s": [n / r["host_s"] for r in rounds], "device_overlaps_per_s": [n / r["device_s"] for r in rounds],
                "parts_of_the_last_device_leg": parts, "kernel_trace": trace_dir,
                "caveat": "the ranks share one device: their device work serialises and every rank ships the whole file over the same link; the "
                          "device leg is the sum of the ranks' work and pessimistic",
            }))


if __name__ == "__main__":
    main()
