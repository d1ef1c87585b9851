"""The layout steps of a round: one rala_hip_layout per component (what Graph::postprocess does without RALA_LAYOUT_BATCH)
against one rala_hip_layout_batch for all of them, in ONE process, on inputs made without a graph (random points, random
adjacency of degree 0-5, k = sqrt(1 / n_c)):

    A   2000 components with sizes log-uniform in 6 .. 2000, 50 steps: launch and sync latency against launches that hold work
    B   one component of 100 000 points, 10 steps: the same arithmetic on both legs, so any loss is a defect

    python tools/layout_batch_bench.py > profiles/r15_layout_batch.txt

Per input: one untimed pass of each leg, then the two legs alternate three times; the outputs of the legs must be equal (==).
Printed: one JSON line per input (both legs' wall times per alternation, rala_hip_get_layout_info's device time and launch
count) and, from a child process of its own under `rocprofv3 --kernel-trace --stats` that runs the batched leg of both inputs
only (--batched-only), the kernel lines of that leg.  (Counters, if wanted, in a run of their own.)"""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rala_amd import hip

T, DT = 0.1, 0.1 / 101


def make_input(sizes, seed):
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.uint32)
    comp_off = np.zeros(len(sizes) + 1, dtype=np.uint32)
    np.cumsum(sizes, out=comp_off[1:])
    n = int(comp_off[-1])
    x, y = rng.random(n), rng.random(n)
    adj_off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(rng.integers(0, 6, size=n), out=adj_off[1:])
    owner = np.repeat(np.arange(len(sizes)), sizes)                    # component of every point
    size_of_entry = np.repeat(sizes[owner], np.diff(adj_off).astype(np.int64))
    adj = (rng.random(int(adj_off[n])) * (size_of_entry + 1)).astype(np.uint32)   # 0 .. n_c (n_c = the origin)
    adj = np.minimum(adj, size_of_entry).astype(np.uint32)
    return comp_off, x, y, adj_off, adj, np.sqrt(1.0 / sizes)


def per_component_leg(ctx, inp, iterations):
    comp_off, x, y, adj_off, adj, k = inp
    gx, gy = x.copy(), y.copy()
    slices = [(int(comp_off[c]), int(comp_off[c + 1])) for c in range(len(k))]
    args = [(gx[lo:hi], gy[lo:hi], adj_off[lo:hi + 1] - adj_off[lo], adj[int(adj_off[lo]):int(adj_off[hi])], float(k[c]))
            for c, (lo, hi) in enumerate(slices)]                      # (slicing is not part of the leg)
    t0 = time.perf_counter()
    for cx, cy, off, a, kc in args:
        ctx.layout(cx, cy, off, a, iterations, kc, T, DT)
    return (time.perf_counter() - t0) * 1e3, gx, gy


def batched_leg(ctx, inp, iterations):
    comp_off, x, y, adj_off, adj, k = inp
    gx, gy = x.copy(), y.copy()
    t0 = time.perf_counter()
    ctx.layout_batch(comp_off, gx, gy, adj_off, adj, k, iterations, T, DT)
    return (time.perf_counter() - t0) * 1e3, gx, gy


def inputs():
    rng = np.random.default_rng(15)
    sizes_a = np.exp(rng.uniform(np.log(6), np.log(2000), size=2000)).astype(np.uint32)
    return (("A", make_input(sizes_a, 1), 50), ("B", make_input([100_000], 2), 10))


def main():
    ctx = hip.Context(0)
    if "--batched-only" in sys.argv:
        for _, inp, iterations in inputs():
            batched_leg(ctx, inp, iterations)
        ctx.close()
        return
    verdict = {}
    for name, inp, iterations in inputs():
        per_component_leg(ctx, inp, iterations)
        batched_leg(ctx, inp, iterations)
        rounds = []
        for _ in range(3):
            ms_single, sx, sy = per_component_leg(ctx, inp, iterations)
            ms_batch, bx, by = batched_leg(ctx, inp, iterations)
            assert (sx == bx).all() and (sy == by).all(), "input %s: the legs' outputs differ" % name
            info = ctx.layout_info()
            rounds.append({"per_component_ms": ms_single, "batched_ms": ms_batch, "batched_device_ms": info["device_ms"],
                           "batched_launches": info["launches"]})
        sizes = np.diff(inp[0])
        single = [r["per_component_ms"] for r in rounds]
        batch = [r["batched_ms"] for r in rounds]
        verdict[name] = (all(b < s for b, s in zip(batch, single)) if name == "A"
                         else all(min(single) <= b <= max(single) or b < min(single) for b in batch))
        print(json.dumps({"input": name, "components": len(sizes), "points": int(sizes.sum()), "iterations": iterations,
                          "per_component_operations": len(sizes) * (iterations + 7), "layout_info": info,
                          "alternations": rounds, "per_component_over_batched": [s / b for s, b in zip(single, batch)],
                          "condition_holds": bool(verdict[name])}))
        sys.stdout.flush()
    ctx.close()
    print(json.dumps({"batched_wins_all_of_A": bool(verdict["A"]), "B_inside_or_below_per_component_spread": bool(verdict["B"])}))
    sys.stdout.flush()
    # the batched leg's kernels: a fresh child under the profiler (this process has closed its context)
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--batched-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            print("rocprofv3 --kernel-trace --stats: no kernel statistics (exit %d)" % r.returncode)
            return
        print("rocprofv3 --kernel-trace --stats, batched leg of A and B (one call each):")
        with open(found[0]) as f:
            for row in csv.DictReader(f):
                kernel = re.search(r"layout_\w+(<\d+>)?", row.get("Name", ""))
                if kernel:
                    print("  %s: calls %s, total %.3f ms, average %.3f ms" % (
                        kernel.group(0), row["Calls"], float(row["TotalDurationNs"]) / 1e6,
                        float(row["AverageNs"]) / 1e6))


if __name__ == "__main__":
    main()
