"""The input stage of `rala --gpus 8` from a BGZF overlap file, host readers against the device ingest in pieces
(RALA_DEVICE_COMPRESSED=1): the figure that would decide the switch's default.

    python tools/ranks_compressed_bench.py [c3] [ranks] > profiles/r14_ranks_compressed.txt

The workload's PAF is written with the repository's generator and compressed as BGZF (members of 65280 bytes of text, zlib
level 6, what `bgzip` writes); the same file is given as the primary file and as `-s`.  The CLI runs with `ranks` ranks (8) that
share device 0 through the in-process transport (RALA_GPUS, RALA_GPU_DEVICES=0,0,..), three alternations of the host leg (switch
off - what such a run gets today, and the yardstick; never the single-context figure) and the device leg (switch on) in one
session.  Timed: the CLI's two `loaded overlaps` stage lines - `[rala::Graph::initialize] loaded overlaps` (the primary file)
and `[rala::Graph::construct] loaded overlaps + [rala::Graph::preprocess]` (the -s file and the step behind it; the step is the
same in both legs) - the process is ended once the second one is out.  Printed: one JSON line.  A later change may turn the
switch on when the device leg wins all three alternations on both lines.

PROXY CAVEAT: all ranks share ONE device here, so their device work - inflate, tokenise - runs one rank after the other, while
the host leg's threads run side by side: the device leg's figure is the SUM of the ranks' work and pessimistic for it.

The kernel lines come from a run of their own: rocprofv3 --kernel-trace --stats -- rala_amd/host/rala --gpus 8 ... with the
switch on (bgzf_inflate_kernel, paf_count_kernel, paf_parse_kernel)."""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rala_amd import build
from rala_amd.cpus import effective_cpus
from rala_amd.synth import Dataset

MEMBER_TEXT = 65280
PRIMARY = "[rala::Graph::initialize] loaded overlaps"
SENSITIVE = "[rala::Graph::construct] loaded overlaps + [rala::Graph::preprocess]"


def member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    total = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1) + body +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def members_of(block):
    return b"".join(member(block[i:i + MEMBER_TEXT]) for i in range(0, len(block), MEMBER_TEXT))


def write_bgzf(src, dst, threads):
    step = MEMBER_TEXT * 256
    with open(src, "rb") as f, open(dst, "wb") as out, ThreadPoolExecutor(threads) as pool:
        while True:
            blocks = [b for b in (f.read(step) for _ in range(threads)) if b]
            if not blocks:
                break
            for m in pool.map(members_of, blocks):
                out.write(m)
        out.write(member(b""))


def leg(exe, fa, gz, ranks, device, threads):
    """-> seconds of the two stage lines"""
    env = dict(os.environ, RALA_COMM="local", RALA_GPUS=str(ranks), RALA_GPU_DEVICES=",".join(["0"] * ranks),
               RALA_DEVICE_COMPRESSED="1" if device else "0")
    p = subprocess.Popen([exe, "-t", str(threads), "-s", gz, fa, gz], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, text=True)
    got = {}
    for line in p.stderr:
        for key in (PRIMARY, SENSITIVE):
            m = re.match(re.escape(key) + r" (\d+\.\d+) s", line)
            if m:
                got[key] = float(m.group(1))
        if SENSITIVE in got:
            break
    p.terminate()
    p.wait()
    if PRIMARY not in got or SENSITIVE not in got:
        raise RuntimeError("rala ended without its stage lines")
    return got[PRIMARY], got[SENSITIVE]


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
    ranks = int(sys.argv[2]) if len(sys.argv) > 2 else 8
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
        write_bgzf(paf, paf + ".gz", threads)
        os.remove(paf)
        print("[ranks_compressed] %s: %.2f GB of PAF as %.2f GB of BGZF in %.1f s" % (wl, text_bytes / 1e9, os.path.getsize(paf + ".gz") / 1e9,
                                                                                    time.time() - t0), file=sys.stderr)
        rounds = []
        for _ in range(3):
            host = leg(exe, fa, paf + ".gz", ranks, False, threads)
            device = leg(exe, fa, paf + ".gz", ranks, True, threads)
            rounds.append({"host_primary_s": host[0], "device_primary_s": device[0], "host_sensitive_s": host[1], "device_sensitive_s": device[1]})
    n = len(ds.overlaps.a_id)
    print(json.dumps({
        "workload": wl, "ranks_on_one_device": ranks, "overlaps": n, "text_bytes": text_bytes, "alternations": rounds,
        "device_wins_all": all(r["device_primary_s"] < r["host_primary_s"] and r["device_sensitive_s"] < r["host_sensitive_s"] for r in rounds),
        "host_primary_overlaps_per_s": [n / r["host_primary_s"] for r in rounds],
        "device_primary_overlaps_per_s": [n / r["device_primary_s"] for r in rounds],
        "caveat": "the ranks share one device: their device work serialises, the device leg is the sum of the ranks' work and pessimistic",
    }))


if __name__ == "__main__":
    main()
