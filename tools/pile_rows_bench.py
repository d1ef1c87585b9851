"""Piles with and without resident rows (option pile_rows), inside ONE process: python tools/pile_rows_bench.py [c3 c5] [alternations]

For every workload the step bench.py times - initialize, construct, transitive reduction - with pile_rows = 1 and 0 in turn,
a fresh context each, at least three alternations.  The modes alternate per LEG (two warm-up steps and five timed ones on one
context), not per step: the option decides what initialize allocates, and a step that first gives back or maps 20 GB of rows
would time the allocator.  Per leg: the step time on the
host's clock, the pile chain's time (rala_hip_timings: pile_ms, events around the chain) and resident_bytes
(rala_hip_get_pile_rows_info).  The comparison that counts is between the legs of one process; the pile_rows = 1 leg is the
parent's bench line.  Rowless legs also time one pass of rala_hip_get_pile_row_digests (every row rebuilt and hashed)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rala_amd import hip
from rala_amd.synth import Dataset

args = sys.argv[1:]
alternations = 3
if args and args[-1].isdigit():
    alternations = max(3, int(args.pop()))
workloads = args or ["c3", "c5"]
STEPS, WARMUP = 5, 2


def leg(ds, rows):
    ctx = hip.Context(0)
    ctx.set_option("pile_rows", rows)
    ctx.set_reads(ds.read_len)
    ctx.set_overlaps(ds.overlaps)

    def step():
        ctx.initialize()
        ctx.construct()
        return ctx.remove_transitive_edges()
    for _ in range(WARMUP):
        n_tr = step()
    step_ms, pile_ms = [], []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        n_tr = step()
        step_ms.append(1e3 * (time.perf_counter() - t0))
        pile_ms.append(float(ctx.timings()["pile_ms"]))
    resident, _ = ctx.pile_rows_info()
    digest_ms = None
    if rows == 0:
        t0 = time.perf_counter()
        fnv, inside, _outside = ctx.pile_row_digests()
        digest_ms = 1e3 * (time.perf_counter() - t0)
    p = ctx.piles()
    sig = (n_tr, int(p["begin"].astype(np.uint64).sum()), int(p["end"].astype(np.uint64).sum()), int(p["median"].astype(np.uint64).sum()),
           int(p["alive"].sum()))
    ctx.close()
    return np.median(step_ms), min(step_ms), np.median(pile_ms), min(pile_ms), resident, digest_ms, sig


for wl in workloads:
    ds = Dataset.config(wl)
    print("%s: %d reads, %d overlaps, %.2f Gbase; %d steps per leg after %d warm-up steps" % (
        wl, ds.n_reads, len(ds.overlaps), float(ds.read_len.astype(np.uint64).sum()) / 1e9, STEPS, WARMUP), flush=True)
    sigs = set()
    for k in range(alternations):
        for rows in (1, 0):
            med, best, pmed, pbest, resident, digest_ms, sig = leg(ds, rows)
            sigs.add(sig)
            print("  %s alternation %d pile_rows=%d: step %.2f ms (best %.2f), pile chain %.2f ms (best %.2f), resident_bytes %d%s" % (
                wl, k, rows, med, best, pmed, pbest, resident, "" if digest_ms is None else ", all rows rebuilt + hashed in %.0f ms" % digest_ms),
                flush=True)
    assert len(sigs) == 1, "the legs disagree on the result: %s" % sorted(sigs)
