"""Helpers of the tests of the layout shared by the ranks (rala_hip_layout_split, rala_hip_mg_layout_batch): the split's rule
in plain Python, from its description in include/rala_hip.h (not by asking the library)."""
TILE = 256


def units(sizes, fused_max):
    """(one behind the unit's last point, cost, is_fused, component) in point order"""
    out, base = [], 0
    for c, n in enumerate(sizes):
        if n and n <= fused_max:
            out.append((base + n, n * n, True, c))
        elif n:
            for first in range(0, n, TILE):
                pts = min(TILE, n - first)
                out.append((base + first + pts, pts * n, False, c))
        base += n
    return out


def split(sizes, fused_max, parts):
    """first_point[parts + 1], cost[parts]: part k ends behind the first unit at which the prefix cost reaches
    ceil(total * (k + 1) / parts), the last part at N"""
    us = units(sizes, fused_max)
    total = sum(u[1] for u in us)
    first, cost = [0], []
    for k in range(parts - 1):
        target = -(-total * (k + 1) // parts)
        prefix, end = 0, 0
        for u in us:
            prefix += u[1]
            end = u[0]
            if prefix >= target:
                break
        else:
            end = sum(sizes)
        first.append(end if us else 0)
    first.append(sum(sizes))
    for k in range(parts):
        cost.append(sum(u[1] for u in us if first[k] < u[0] <= first[k + 1]))
    return first, cost


def share(sizes, fused_max, parts, rank):
    """what rank `rank` of `parts` owns: the fields of rala_hip_mg_layout_info that follow from the split"""
    first, cost = split(sizes, fused_max, parts)
    lo, hi = first[rank], first[rank + 1]
    mine = [u for u in units(sizes, fused_max) if lo < u[0] <= hi]
    return {"first_point": lo, "end_point": hi,
            "components_fused_256": sum(1 for u in mine if u[2] and sizes[u[3]] <= 256),
            "components_fused_1024": sum(1 for u in mine if u[2] and sizes[u[3]] > 256),
            "step_tiles": sum(1 for u in mine if not u[2]), "cost": cost[rank], "total_cost": sum(cost)}
