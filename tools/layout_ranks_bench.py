"""What sharing a round's layout out over ranks COSTS, on one device: rala_hip_layout_batch on one context (the yardstick)
against rala_hip_mg_layout_batch_threads with 8 ranks that all sit on device 0 and exchange through the in-process transport,
in ONE process, on the inputs A and B of tools/layout_batch_bench.py.

    python tools/layout_ranks_bench.py > profiles/r22_layout_ranks.txt

On one device the ranks' kernels serialise: the collective leg's time is the SUM of the ranks' work plus the exchanges.  The
ratio prices the overhead - eight uploads of the whole batch, a host rendezvous and device-to-device copies per step, launches
that fill an eighth of the device each -; it is NOT a scaling figure, and no threshold is set for it.

Per input: one untimed pass of each leg, then the two legs alternate three times; the outputs of the legs must be equal (as
bytes).  Printed: one JSON line per input with both legs' wall times per alternation, their ratio, and every rank's
rala_hip_mg_get_layout_info of the last collective call."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rala_amd import hip

from layout_batch_bench import DT, T, batched_leg, inputs

WORLD = 8


def ranks_leg(ranks, inp, iterations):
    comp_off, x, y, adj_off, adj, k = inp
    gx, gy = x.copy(), y.copy()
    t0 = time.perf_counter()
    hip.layout_ranks(ranks, comp_off, gx, gy, adj_off, adj, k, iterations, T, DT)
    return (time.perf_counter() - t0) * 1e3, gx, gy


def main():
    ctx = hip.Context(0)
    group = hip.LocalGroup(WORLD)
    ranks = [hip.ShardedRank(0, r, WORLD, group) for r in range(WORLD)]
    for name, inp, iterations in inputs():
        batched_leg(ctx, inp, iterations)
        ranks_leg(ranks, inp, iterations)
        rounds = []
        for _ in range(3):
            ms_one, bx, by = batched_leg(ctx, inp, iterations)
            ms_ranks, rx, ry = ranks_leg(ranks, inp, iterations)
            assert bx.tobytes() == rx.tobytes() and by.tobytes() == ry.tobytes(), "input %s: the legs' outputs differ" % name
            rounds.append({"one_context_ms": ms_one, "eight_ranks_one_device_ms": ms_ranks, "ranks_over_one_context": ms_ranks / ms_one})
        print(json.dumps({"input": name, "components": len(inp[5]), "points": int(inp[0][-1]), "iterations": iterations,
                          "ranks": WORLD, "transport": "local, all ranks on device 0", "outputs_equal": True,
                          "alternations": rounds, "one_context_layout_info": ctx.layout_info(),
                          "rank_layout_info": [r.layout_info() for r in ranks]}))
        sys.stdout.flush()
    for r in ranks:
        r.close()
    group.close()
    ctx.close()


if __name__ == "__main__":
    main()
