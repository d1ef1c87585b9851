"""Designed repeat hills for the sensitive pass, and a plain model of it that names every branch it takes.

The model (`find_hills`, `bridge`, `keeps`, `trace`) restates Pile::find_repetitive_hills, Pile::check_repetitive_hills and
Pile::is_valid_overlap (reference pile.cpp:500-630) and the two loops that call them (graph.cpp:1028-1051) in Python ints and
floats with the same truncations.  It takes what the oracle has - a row, its slope regions at 1.42, region, median, p10, the
component's median, the trimmed sensitive dovetails, the surviving primary overlaps - and returns the hills, their flags and
the overlaps the filter removes, and for every comparison it made (decision, side, margin): margin 0 is the last integer on
that side of the comparison.  tests/test_repcase_cpu.py shows that the model and the oracle agree on every case, and counts
which decisions the cases reach on which side; tests/test_gpu_repeats.py runs the cases on the device.

Layer A: handmade piles for rala_hip_find_repetitive_hills - one read per call, floors and plateaus from whole-read and short
records against throw-away partners (as tests/sawcase.py makes them), every value designed in integers.
Layer B: the generator's sensitive set of three generated data sets plus designed records: stacks of records on [x, y) of a
target lay a plateau of exactly their number there (graph.cpp:929-938 adds the bounds whether or not the record survives
trim), designed dovetails bridge a hill or fail to by one base.  A designed dovetail is a long live read's suffix on the
target's prefix (or its prefix on the target's suffix), typed kAB / kBA by the oracle's Overlap::trim and type before it is
taken.  It is not a copy of one of the target's surviving primary dovetails with one end moved: the hills that only the
designed dovetail may bridge reach past every generated dovetail, up to 0.8 of the target, so the copy's moved end would be
thousands of bases from where its query side ends, and whether the result is still a dovetail is the oracle's to say either
way; a query chosen for its length keeps the 5 % and 12.5 % rules of Overlap::type out of the way.  The builder runs the oracle and moves a plateau by the difference it reads; what a case is, is the oracle's verdict
(test_repcase_cpu.py), never the intention.
"""
import math

import numpy as np

from rala_amd.synth import Dataset, Overlaps, FIELDS

kFuzz = 420
kWindow = 847

# decisions (the census of tests/test_repcase_cpu.py wants each on every side)
MEDIAN_SWITCH = "median > 1.42 * dataset median"              # taken / not
MAX_OPERAND = "max(dataset median, p10)"                      # dm / p10
CENTRES = "slope centres > 0.84 * span"                       # refused / passed
PEAK = "peak above 1.42 * max(ends)"                          # found / none
SHARE = "valid points < 0.9 * gap"                            # refused / passed
MERGE = "intervalMerge"                                       # absorbed / apart
CLAMP_BEGIN = "clamp at begin"                                # clamped / inside
CLAMP_END = "clamp at end"                                    # clamped / inside
EDGE_LEFT = "hill.first < 0.1 * span + begin"                 # left / not
EDGE_RIGHT = "hill.second > 0.9 * span + begin"               # right / not
CLASS = "hill class"                                          # left / right / neither / both
TIE = "begin - begin_ == end_ - end"                          # tie / apart
BRIDGE_LEFT = "bridge: end >= hill.second + 420"              # bridged / short
BRIDGE_RIGHT = "bridge: begin + 420 <= hill.first"            # bridged / short
FILTER_LEFT_A = "filter, a side: end < hill.second + 420"     # removed / kept
FILTER_LEFT_B = "filter, b side: end < hill.second + 420"
FILTER_RIGHT_A = "filter, a side: begin + 420 > hill.first"
FILTER_RIGHT_B = "filter, b side: begin + 420 > hill.first"
UNBRIDGED = "filter meets an unbridged edge hill"             # kept (the only side there is)

SIDES = {
    MEDIAN_SWITCH: ("taken", "not"), MAX_OPERAND: ("dm", "p10"), CENTRES: ("refused", "passed"), PEAK: ("found", "none"),
    SHARE: ("refused", "passed"), MERGE: ("absorbed", "apart"), CLAMP_BEGIN: ("clamped", "inside"),
    CLAMP_END: ("clamped", "inside"), EDGE_LEFT: ("left", "not"), EDGE_RIGHT: ("right", "not"),
    CLASS: ("left", "right", "neither", "both"), TIE: ("tie", "apart"), BRIDGE_LEFT: ("bridged", "short"),
    BRIDGE_RIGHT: ("bridged", "short"), FILTER_LEFT_A: ("removed", "kept"), FILTER_LEFT_B: ("removed", "kept"),
    FILTER_RIGHT_A: ("removed", "kept"), FILTER_RIGHT_B: ("removed", "kept"), UNBRIDGED: ("kept",),
}
# placed by geometry: the smallest margin on every side is 0 or 1
PLACED = (CENTRES, PEAK, SHARE, CLAMP_BEGIN, CLAMP_END, EDGE_LEFT, EDGE_RIGHT, TIE, BRIDGE_LEFT, BRIDGE_RIGHT, FILTER_LEFT_A,
          FILTER_LEFT_B, FILTER_RIGHT_A, FILTER_RIGHT_B)
# these depend on medians: Layer A places them, Layer B only has to reach both sides
BY_MEDIANS = (MEDIAN_SWITCH, MAX_OPERAND)


# ---- margins: x is an integer, t what it is compared with; 0 = x is the last integer on its side -------------------------------
def _gt(x, t):
    """x > t -> (taken, margin)"""
    f = math.floor(t)
    return (True, x - (f + 1)) if x > t else (False, f - x)


def _lt(x, t):
    """x < t"""
    c = math.ceil(t)
    return (True, c - 1 - x) if x < t else (False, x - c)


def _ge(x, t):
    """x >= t, both integers"""
    return (True, x - t) if x >= t else (False, t - 1 - x)


def _u32(x):
    return int(x) & 0xFFFFFFFF


# A deliberately wrong model: TWEAK[decision] = +1 / -1 moves that compare's threshold by one unit, TWEAK["0.336"] replaces the
# factor, TWEAK["peak end"] takes the peak value from the up region's end alone.  tests/test_repcase_cpu.py shows that every
# such model differs from the oracle on some case: the decision is not only reached with margin 0, its outcome shows in the
# hills, the flags or the surviving overlaps.
TWEAK = {}


def _tw(decision):
    return TWEAK.get(decision, 0)


# ---- Pile::find_repetitive_hills (pile.cpp:500-566) ----------------------------------------------------------------------------
def interval_merge(iv, log=None):
    """intervalMerge (pile.cpp:31-52): interval i absorbs, in index order, every later or earlier one it touches - as it has
    grown by then"""
    iv = [list(p) for p in iv]
    merged = [False] * len(iv)
    out = []
    for i in range(len(iv)):
        if merged[i]:
            continue
        for j in range(len(iv)):
            if i == j or merged[j]:
                continue
            if iv[i][0] < iv[j][1] and iv[i][1] > iv[j][0]:
                if log is not None:
                    log.append((MERGE, "absorbed", min(iv[j][1] - iv[i][0], iv[i][1] - iv[j][0]) - 1))
                merged[j] = True
                iv[i][0] = min(iv[i][0], iv[j][0])
                iv[i][1] = max(iv[i][1], iv[j][1])
            elif log is not None:
                log.append((MERGE, "apart", max(iv[i][0] - iv[j][1], iv[j][0] - iv[i][1])))
        out.append((iv[i][0], iv[i][1]))
    return out


def find_hills(row, slopes, begin, end, median, p10, dataset_median, log):
    """the hills Pile::find_repetitive_hills(dataset_median) adds to a pile without any; slopes: (first << 1 | is_up, last)"""
    row = np.asarray(row)
    dm = int(dataset_median)
    taken, m = _gt(int(median), 1.42 * dm)
    log.append((MEDIAN_SWITCH, "taken" if taken else "not", m))
    if taken:
        log.append((MAX_OPERAND, "dm" if dm >= int(p10) else "p10", abs(dm - int(p10))))
        dm = max(dm, int(p10))
    R = [(int(k), int(l)) for k, l in slopes]
    if not R:
        return []
    raw = []
    span = int(end) - int(begin)
    for i in range(len(R) - 1):
        if not R[i][0] & 1:
            continue
        u_first, u_last = R[i][0] >> 1, R[i][1]
        for j in range(i + 1, len(R)):
            if R[j][0] & 1:
                continue
            w_first, w_last = R[j][0] >> 1, R[j][1]
            far, m = _gt(_u32((w_first + w_last) // 2 - (u_first + u_last) // 2), 0.84 * span + _tw(CENTRES))
            log.append((CENTRES, "refused" if far else "passed", m))
            if far:
                continue
            ends = (int(row[u_last]), int(row[w_first]))
            peak = int(1.42 * (ends[0] if TWEAK.get("peak end") else max(ends))) + _tw(PEAK)
            floor_v = int(dm * 1.42)
            inner = row[u_last + 1:w_first] if w_first > u_last + 1 else row[:0]
            found, m = _gt(int(inner.max()) if len(inner) else 0, peak)
            log.append((PEAK, "found" if found else "none", m))
            if not found:
                continue
            valid = int((inner > floor_v).sum())
            few, m = _lt(valid, 0.9 * _u32(w_first - u_last) + _tw(SHARE))
            log.append((SHARE, "refused" if few else "passed", m))
            if few:
                continue
            k = TWEAK.get("0.336", 0.336)
            raw.append((_u32(int(u_last - k * _u32(u_last - u_first))), _u32(int(w_first + k * _u32(w_last - w_first)))))
    hills = []
    for first, second in interval_merge(raw, log):
        log.append((CLAMP_BEGIN, "clamped", begin - first - 1) if first < begin else (CLAMP_BEGIN, "inside", first - begin))
        log.append((CLAMP_END, "clamped", second - end - 1) if second > end else (CLAMP_END, "inside", end - second))
        hills.append((max(int(begin) + _tw(CLAMP_BEGIN), first), min(int(end) + _tw(CLAMP_END), second)))
    return hills


def hill_class(hill, begin, end, log=None):
    """(is left, is right) by the two edge compares of check_repetitive_hills / is_valid_overlap"""
    span = int(end) - int(begin)
    left, ml = _lt(hill[0], 0.1 * span + begin + _tw(EDGE_LEFT))
    right, mr = _gt(hill[1], 0.9 * span + begin + _tw(EDGE_RIGHT))
    if log is not None:
        log.append((EDGE_LEFT, "left" if left else "not", ml))
        log.append((EDGE_RIGHT, "right" if right else "not", mr))
        log.append((CLASS, "both" if left and right else "left" if left else "right" if right else "neither", 0))
    return left, right


def bridge(hills, begin, end, dovetails, log):
    """Pile::check_repetitive_hills (pile.cpp:568-592) for every trimmed sensitive dovetail (b_begin, b_end) on this target"""
    flags = [0] * len(hills)
    for x, y in dovetails:
        for i, h in enumerate(hills):
            if not (x < h[1] and h[0] < y):
                continue
            left, right = hill_class(h, begin, end)
            front, back = _u32(x - begin) + _tw(TIE), _u32(end - y)
            if left or right:
                log.append((TIE, "tie", 0) if front == back else (TIE, "apart", abs(front - back) - 1))
            if left and front < back:
                ok, m = _ge(y, h[1] + kFuzz + _tw(BRIDGE_LEFT))
                log.append((BRIDGE_LEFT, "bridged" if ok else "short", m))
                if ok:
                    flags[i] = 1
            elif right and front > back:
                ok, m = _ge(h[0], x + kFuzz + _tw(BRIDGE_RIGHT))
                log.append((BRIDGE_RIGHT, "bridged" if ok else "short", m))
                if ok:
                    flags[i] = 1
    return flags


def keeps(hills, flags, begin, end, x, y, side, log):
    """Pile::is_valid_overlap(x, y) (pile.cpp:605-630); side: 'a' or 'b' of the primary overlap"""
    for i, h in enumerate(hills):
        if not (x < h[1] and h[0] < y):
            continue
        left, right = hill_class(h, begin, end)
        if left:
            if not flags[i]:
                log.append((UNBRIDGED, "kept", 0))
                continue
            which = FILTER_LEFT_A if side == "a" else FILTER_LEFT_B
            inside, m = _lt(y, h[1] + kFuzz + _tw(which))
            log.append((which, "removed" if inside else "kept", m))
            if inside:
                return False
        elif right:
            if not flags[i]:
                log.append((UNBRIDGED, "kept", 0))
                continue
            which = FILTER_RIGHT_A if side == "a" else FILTER_RIGHT_B
            inside, m = _gt(x + kFuzz + _tw(which), h[0])
            log.append((which, "removed" if inside else "kept", m))
            if inside:
                return False
    return True


class Trace:
    """what the model found for one case set: hills / flags per read, kept[k] per primary overlap, log[read] = decisions"""

    def __init__(self):
        self.hills, self.flags, self.log, self.kept = {}, {}, {}, None

    def decisions(self):
        for r in sorted(self.log):
            for d in self.log[r]:
                yield d

    def describe(self, r):
        lines = ["read %d: hills %s flags %s" % (r, self.hills.get(r, []), self.flags.get(r, []))]
        lines += ["    %-48s %-8s margin %d" % d for d in self.log.get(r, [])]
        return "\n".join(lines)


def components(n, a, b, median):
    """comp_median[r] of every read an overlap touches (graph.cpp:971-1014): element at size / 2 of the sorted medians"""
    parent = np.arange(n)

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = root(x), root(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    groups = {}
    for r in np.unique(np.concatenate((a, b))).tolist():
        groups.setdefault(root(r), []).append(r)
    out, size = {}, {}
    for members in groups.values():
        m = int(np.sort(median[members])[len(members) // 2])
        for r in members:
            out[r], size[r] = m, len(members)
    return out, size


def trace(rows, slopes, piles, comp_median, dovetails, primaries):
    """The whole pass: rows[r], slopes[r] for the reads of comp_median (read -> its component's median); piles: begin, end,
    median, p10; dovetails(read): [(b_begin, b_end)] of the trimmed sensitive dovetails on it, in file order;
    primaries: a_id, b_id, a_begin, a_end, b_begin, b_end of the surviving overlaps."""
    t = Trace()
    for r, dm in comp_median.items():
        log = t.log.setdefault(r, [])
        B, E = int(piles["begin"][r]), int(piles["end"][r])
        t.hills[r] = find_hills(rows[r], slopes[r], B, E, int(piles["median"][r]), int(piles["p10"][r]), dm, log)
        for h in t.hills[r]:
            hill_class(h, B, E, log)
        t.flags[r] = bridge(t.hills[r], B, E, dovetails(r), log) if t.hills[r] else []
    n = len(primaries["a_id"])
    t.kept = np.ones(n, dtype=bool)
    for k in range(n):
        for side in "ab":
            r = int(primaries[side + "_id"][k])
            if not t.hills.get(r):
                continue
            B, E = int(piles["begin"][r]), int(piles["end"][r])
            if not keeps(t.hills[r], t.flags[r], B, E, int(primaries[side + "_begin"][k]), int(primaries[side + "_end"][k]), side,
                         t.log[r]):
                t.kept[k] = False
                break                   # (is_valid_overlap of b is not asked when a's says no: graph.cpp:1046-1047)
    return t


# ---- the oracle's side of a case set -------------------------------------------------------------------------------------------
def concat(*sets):
    return Overlaps(**{f: np.concatenate([getattr(s, f) for s in sets]) for f in FIELDS},
                    strand=np.concatenate([s.strand for s in sets]))


def records(rows):
    """Overlaps from (a, b, a_begin, a_end, b_begin, b_end, strand) tuples"""
    a = np.array(rows, dtype=np.int64).reshape(-1, 7)
    return Overlaps(a_id=a[:, 0], b_id=a[:, 1], a_begin=a[:, 2], a_end=a[:, 3], b_begin=a[:, 4], b_end=a[:, 5],
                    length=np.maximum(a[:, 3] - a[:, 2], a[:, 5] - a[:, 4]), strand=a[:, 6])


class Front:
    """the oracle behind preprocess_chimeras on a data set: what the sensitive records are designed against"""

    def __init__(self, ds, ref=False):
        from oracle.oracle import Oracle
        self.ds = ds
        self.o = o = Oracle(ds.read_len, ds.overlaps, n_threads=8, ref=ref)
        assert o.initialize() == 0
        o.pass2()
        o.preprocess_chimeras()
        self.piles = o.piles()
        self.ov = o.overlap_list(0)
        src = self.ov["src"].astype(np.int64)
        self.ov["a_id"], self.ov["b_id"] = ds.overlaps.a_id[src].astype(np.int64), ds.overlaps.b_id[src].astype(np.int64)


def sensitive_pass(ds, sens, ref=False):
    """the oracle through preprocess_repeats, and the model on what it holds then; returns (state, trace)"""
    f = Front(ds, ref)
    o, n = f.o, ds.n_reads
    o.preprocess_repeats(sens)
    st = {"front": f, "oracle": o, "piles": o.piles(), "rep": o.all_intervals(2), "ov": o.overlap_list(0)}
    flags = [o.repeat_flags(r) for r in range(n)]
    st["flags"] = np.concatenate(flags) if flags else np.zeros(0, np.uint8)
    p = st["piles"]
    comp, st["comp_size"] = components(n, f.ov["a_id"], f.ov["b_id"], p["median"])
    st["comp_median"] = comp
    rows, slopes = {}, {}
    for r in comp:
        slopes[r] = o.find_slopes(r, 1.42)
        rows[r] = o.pile_data(r) if len(slopes[r]) else None
    by_target = {}
    order = np.argsort(sens.b_id, kind="stable")
    cuts = np.searchsorted(sens.b_id[order], np.arange(n + 1))

    def dovetails(r):
        """the records on target r that survive trim as kAB / kBA (graph.cpp:1028-1038), trimmed, in file order"""
        if r not in by_target:
            out = []
            B = int(p["begin"][r])
            for i in order[cuts[r]:cuts[r + 1]].tolist():
                c = [int(sens.a_begin[i]), int(sens.a_end[i]), int(sens.b_begin[i]) + B, int(sens.b_end[i]) + B, int(sens.length[i])]
                ok, c, t = o.overlap_trim_type(int(sens.a_id[i]), r, int(sens.strand[i]), c)
                if ok and t in (3, 4):
                    out.append((int(c[2]), int(c[3])))
            by_target[r] = out
        return by_target[r]

    st["dovetails"] = dovetails
    st["again"] = lambda: trace(rows, slopes, p, comp, dovetails, f.ov)
    return st, st["again"]()


def verdict(st, t):
    """None when the model's hills, flags and surviving overlaps are the oracle's, else what differs first"""
    offs, pairs = st["rep"]
    for r in range(len(offs) - 1):
        want = [tuple(int(v) for v in x) for x in pairs[int(offs[r]):int(offs[r + 1])]]
        got = t.hills.get(r, [])
        if want != got:
            return "hills of read %d: oracle %s\n%s" % (r, want, t.describe(r))
        wf = st["flags"][int(offs[r]):int(offs[r + 1])].tolist()
        if wf != list(t.flags.get(r, [])):
            return "flags of read %d: oracle %s\n%s" % (r, wf, t.describe(r))
    kept = st["front"].ov["src"][t.kept]
    if len(kept) != len(st["ov"]["src"]) or (kept != st["ov"]["src"]).any():
        gone_o = set(st["front"].ov["src"].tolist()) - set(st["ov"]["src"].tolist())
        gone_m = set(st["front"].ov["src"][~t.kept].tolist())
        k = sorted(gone_o ^ gone_m)[0]
        i = int(np.nonzero(st["front"].ov["src"] == k)[0][0])
        a, b = int(st["front"].ov["a_id"][i]), int(st["front"].ov["b_id"][i])
        return "overlap %d (%d, %d): removed by the oracle %s, by the model %s\n%s\n%s" % (
            k, a, b, k in gone_o, k in gone_m, t.describe(a), t.describe(b))
    return None


# ---- Layer A: handmade piles, one read per call of rala_hip_find_repetitive_hills ------------------------------------------------
kEdge = 15              # Graph::initialize shrinks every record by 15 bases on either side (graph.cpp:317-324)
kPartnerLen = 3000


def _flat(length, floor):
    row = np.zeros(length, dtype=np.int64)
    row[kEdge:length - kEdge] = floor
    return row


def _layers(row):
    """[s, e) intervals whose sum is the row (nested: the last one opened closes first)"""
    stack, out, prev = [], [], 0
    step = np.diff(np.concatenate(([0], row, [0])))
    for p in np.nonzero(step)[0].tolist():
        v = prev + int(step[p])
        if v > prev:
            stack += [p] * (v - prev)
        else:
            out += [(stack.pop(), p) for _ in range(prev - v)]
        prev = v
    return out


class Call:
    """one call: the read, begin / end / dataset median as given; median, p10 and the model's view are filled by the builder"""

    def __init__(self, name, row, begin=None, end=None, dm=10):
        self.name, self.row, self.dm = name, row, dm
        self.begin = kEdge if begin is None else begin
        self.end = len(row) - kEdge if end is None else end

    def model(self, log):
        return find_hills(self.shrunk(), self.slopes, self.begin, self.end, self.median, self.p10, self.dm, log)

    def shrunk(self):
        """the row as Pile::shrink leaves it for [begin, end) (pile.cpp:311-318)"""
        row = self.row.copy()
        row[:self.begin] = 0
        row[self.end:] = 0
        return row.astype(np.uint16)


class _Scratch:
    """one oracle pile to try a row on: median, p10, slopes - and the model's hills and decisions from them"""

    def __init__(self, ref=False):
        self.ref, self.o, self.length = ref, None, 0

    def look(self, call):
        from oracle.oracle import Oracle
        if self.o is None or self.length != len(call.row):
            self.length = len(call.row)
            self.o = Oracle(np.array([self.length], dtype=np.uint32), None, ref=self.ref)
        o = self.o
        row = call.shrunk()
        o.set_pile_state(0, row, call.begin, call.end)
        o.find_median(0)
        p = o.piles()
        call.median, call.p10 = int(p["median"][0]), int(p["p10"][0])
        call.log = []
        call.slopes = o.find_slopes(0, 1.42)
        call.hills = call.model(call.log)
        return call


def _side(call, decision):
    return [(s, m) for d, s, m in call.log if d == decision]


def _search(scratch, make, values, decision, side):
    """the first value v for which make(v)'s model log has `decision` on `side` with margin 0"""
    for v in values:
        c = scratch.look(make(v))
        if (side, 0) in _side(c, decision):
            return c
    raise AssertionError("no value puts %r on side %r with margin 0" % (decision, side))


def _layer_a_calls():
    s = _Scratch()
    L, f = 12000, 10
    calls = []

    def plateau(floor, height, at, length=L):
        row = _flat(length, floor)
        row[at[0]:at[1]] = height
        return row

    calls.append(Call("one plateau", plateau(f, 30, (4000, 6000))))
    # the up slope at 3000 exists because of what lies 847 bases on; what lies between it and the dip at 3400 is at
    # 1.42 * max(ends) or one above; behind the dip too few points are valid for the pairs that end behind the 16s
    for m in (14, 15):
        row = _flat(L, f)
        row[3001:3400] = m
        row[3400:3405] = 7
        row[3405:3847] = 12
        row[3847:4847] = 16
        calls.append(Call("between the slopes at %d (peak value 14)" % m, row, dm=9))       # (14 > uint32(9 * 1.42): valid points)
    # ... and the mirror image: the down slope at 4999 exists because of what lies 847 bases back, the larger end is w_first
    for m in (14, 15):
        row = _flat(L, f)
        row[3153:4153] = 16
        row[4153:4595] = 12
        row[4595:4600] = 7
        row[4600:4999] = m
        calls.append(Call("between the slopes at %d (peak value 14), mirrored" % m, row, dm=9))
    # a plateau at uint32(dm * 1.42) = 14 and one above: no point between the slopes counts, or all do
    for h in (14, 15):
        calls.append(Call("plateau at %d over floor 6, dataset median 10" % h, plateau(6, h, (4000, 6000))))
    # two plateaus of 4000, the floor between them: the outer pair's valid points on either side of 0.9 * gap
    def two(g):
        row = _flat(13000, f)
        row[2000:6000] = 30
        row[6000 + g:10000 + g] = 30
        return Call("two plateaus %d apart" % g, row)
    a = _search(s, two, range(880, 896), SHARE, "passed")
    b = _search(s, two, range(880, 896), SHARE, "refused")
    calls += [a, b]
    # a staircase: several up regions before the first down region, many pairs, one merge
    row = _flat(L, f)
    for k, h in enumerate((15, 22, 32, 46)):
        row[3000 + 1000 * k:8000] = h
    calls.append(Call("staircase up", row))
    row = _flat(L, f)
    for k, h in enumerate((15, 22, 32, 46)):
        row[3000:8000 - 1000 * k] = h
    calls.append(Call("staircase down", row))
    row = _flat(L, f)
    row[2000:3000] = 30
    row[4200:5200] = 16
    row[4500:4900] = 40
    row[7000:9000] = 25
    calls.append(Call("three hills, the middle one with a step", row))
    # a wide plateau: the slope centres 0.84 * (end - begin) apart, end moved by one base
    wide = plateau(f, 30, (1000, 10000))
    calls.append(_search(s, lambda e: Call("wide plateau, end %d" % e, wide, end=e), range(11730, 11746), CENTRES, "refused"))
    calls.append(_search(s, lambda e: Call("wide plateau, end %d" % e, wide, end=e), range(11730, 11746), CENTRES, "passed"))
    # begin / end cut into the hill: the cut makes slopes of its own (the row is zero outside), the hill is clamped by a lot
    mid = plateau(f, 30, (3000, 6000))
    calls.append(Call("begin cuts into the hill's front", mid, begin=2715))
    calls.append(Call("end cuts into the hill's back", mid, end=6250))
    calls.append(Call("begin and end inside the plateau", mid, begin=3500, end=5500))
    # ... and by one base or none: a plateau that begins with the coverage, 15 bases in (the up region is [0, 14], the hill
    # begins at 9), and one that ends with it; begin and end around the hill's ends, in the zeroes
    front, back = plateau(f, 30, (kEdge, 3000)), plateau(f, 30, (9000, L - kEdge))
    for side in ("clamped", "inside"):
        calls.append(_search(s, lambda b: Call("begin %d, the hill begins at 9" % b, front, begin=b), range(0, 15), CLAMP_BEGIN, side))
        calls.append(_search(s, lambda e: Call("end %d, the hill ends at %d" % (e, L - 11), back, end=e), range(L - 14, L + 1),
                             CLAMP_END, side))
    # median > 1.42 * dataset median: floor 21 (the median), a shoulder at 14 or at 8 over the first eighth (p10), or none
    for shoulder in (14, 8, None):
        row = plateau(21, 50, (5000, 7000))
        if shoulder:
            row[kEdge:1500] = shoulder
        for dm in (12, 13, 14, 15, 16):
            calls.append(Call("median 21, p10 %d, dataset median %d" % (shoulder or 21, dm), row, dm=dm))
    # 1.42 * 50 is 71 on paper and in double; the median is 71
    for dm in (49, 50):
        calls.append(Call("median 71, dataset median %d" % dm, plateau(71, 160, (5000, 7000)), dm=dm))
    for c in calls:
        s.look(c)
    return calls


class LayerA:
    """read k is calls[k]'s, the partners follow"""

    def __init__(self):
        self.calls = _layer_a_calls()
        n = len(self.calls)
        rows = []
        n_partners = 0
        for t, c in enumerate(self.calls):
            c.read = t
            mine = _layers(c.row)
            n_partners = max(n_partners, len(mine))
            for k, (b, e) in enumerate(mine):
                rows.append((t, n + k, b - kEdge, e + kEdge, 0, min(e - b + 2 * kEdge, kPartnerLen), k & 1))
        self.read_len = np.array([len(c.row) for c in self.calls] + [kPartnerLen] * n_partners, dtype=np.uint32)
        self.n_reads = len(self.read_len)
        self.overlaps = records(rows)


_layer_a = []


def layer_a():
    if not _layer_a:
        _layer_a.append(LayerA())
    return _layer_a[0]


def oracle_call(call, ref=False):
    """Pile::find_repetitive_hills on a fresh pile with the call's state: (hills, flags)"""
    from oracle.oracle import Oracle
    o = Oracle(np.array([len(call.row)], dtype=np.uint32), None, ref=ref)
    o.set_pile_state(0, call.shrunk(), call.begin, call.end)
    o.find_median(0)
    p = o.piles()
    assert (int(p["median"][0]), int(p["p10"][0])) == (call.median, call.p10)
    o.find_repetitive_hills(0, call.dm)
    return [tuple(int(v) for v in x) for x in o.intervals(0, 2)], o.repeat_flags(0).tolist()


# ---- Layer B: designed sensitive records on generated sets -----------------------------------------------------------------------
# named for the kernels their designed targets start in (CaseSet.tiers; tests/test_repcase_cpu.py asserts them)
BASES = {"cap2048": (600, 60_000, 9), "position": (900, 30_000, 4), "cap512_cap1024": (5000, 1_000_000, 7)}
kMaxTargets = 8
kUp, kDown = 286, 284       # a plateau [x, y) of a flat stretch makes the hill [x - 286, y + 284]: 0.336 of the slope regions


kCaps = (510, 1022, 2046)      # events a read may have in the cap-512 / cap-1024 / cap-2048 run-space kernels (sens_split_kernel)
TIERS = ("cap 512", "cap 1024", "cap 2048", "position space")


def events(ds, sens):
    """per read what sens_split_kernel counts: two events per primary record the read is in, two per sensitive record on it"""
    n = ds.n_reads
    ov = ds.overlaps
    return 2 * (np.bincount(ov.a_id, minlength=n) + np.bincount(ov.b_id, minlength=n) + np.bincount(sens.b_id, minlength=n))


def tier(read_len, ev):
    """the kernel a read of the sensitive pass starts in (reads of up to 16384 bases; the longer ones have classes of their own)"""
    assert read_len <= 16384
    return TIERS[sum(ev > c for c in kCaps)]


class Builder:
    """One base set.  Runs the oracle with the generator's sensitive set, then designs plateaus and dovetails on chosen targets
    against what it read: rows, regions, the generator's own dovetails, the surviving primary overlaps.  A plateau is tried on a
    scratch pile (oracle slopes, model hills) and moved by the difference; the oracle's verdict on the whole set comes after."""

    def __init__(self, name):
        self.name = name
        self.ds = ds = Dataset(*BASES[name])
        f = Front(ds)
        self.gen = ds.sensitive(f.piles["alive"], f.piles["begin"], f.piles["end"])
        self.st, _ = sensitive_pass(ds, self.gen)
        self.front = f = self.st["front"]
        self.piles = self.st["piles"]
        self.B, self.E = self.piles["begin"].astype(np.int64), self.piles["end"].astype(np.int64)
        self.S = self.E - self.B
        comp = self.st["comp_median"]
        # (fewest events first: the tiers of the run-space kernels go by events, and a stack adds two per record)
        self.base_events = events(ds, self.gen)
        self.candidates = sorted((r for r in sorted(comp) if self.S[r] > 8000), key=lambda r: (int(self.base_events[r]), r))
        self.used, self.roles, self.rows, self.partners, self.want, self._height = [], {}, [], set(), None, {}
        self.scratch = _Scratch()
        # queries for the designed records: the longest live reads
        live = np.nonzero(self.piles["alive"])[0]
        self.queries = [int(r) for r in live[np.argsort(-self.S[live], kind="stable")][:12]]

    # -- what the target looks like
    def base_row(self, r):
        return self.st["oracle"].pile_data(r).astype(np.int64)

    def primaries(self, r, side):
        """(begin, end, partner) of the surviving primary overlaps with r on `side` whose other read is no target"""
        ov = self.front.ov
        k = np.nonzero(ov[side + "_id"] == r)[0]
        other = "b" if side == "a" else "a"
        return [(int(ov[side + "_begin"][i]), int(ov[side + "_end"][i]), int(ov[other + "_id"][i])) for i in k
                if int(ov[other + "_id"][i]) not in self.used]

    def generator_dovetails(self, r):
        return self.st["dovetails"](r)

    def height(self, r):
        """records in a stack: the plateau has to be above 1.42 times whatever lies beside it and above uint32(1.42 * component
        median) - a little over 0.45 of the coverage, no more: every record is two events, and the tiers go by events"""
        if r in self._height:
            return self._height[r]
        row = self.base_row(r)[self.B[r] + 200:self.E[r] - 200]
        self._height[r] = max(int(0.45 * int(row.max())) + 8, int(1.42 * self.st["comp_median"][r]) + 8 - int(row.min()))
        return self._height[r]

    def look(self, r, plateaus):
        row = self.base_row(r)
        for x, y, *k in plateaus:
            row[self.B[r] + x:self.B[r] + y] += k[0] if k else self.height(r)
        c = Call("", row, int(self.B[r]), int(self.E[r]), dm=self.st["comp_median"][r])
        return self.scratch.look(c)

    def place(self, r, x, y, first=None, second=None):
        """[x, y) (trimmed coordinates) moved until the hill over it begins at `first` / ends at `second` (absolute)"""
        for _ in range(6):
            c = self.look(r, [(x, y)])
            h = [h for h in c.hills if h[0] <= self.B[r] + x and h[1] >= self.B[r] + y]
            if len(h) != 1:
                return None
            dx = 0 if first is None else first - h[0][0]
            dy = 0 if second is None else second - h[0][1]
            if dx == 0 and dy == 0:
                return x, y, h[0]
            x, y = x + dx, y + dy
            if not (0 < x < y < self.S[r]):
                return None
        return None

    # -- designed records
    def stack(self, r, x, y, k=None):
        k = k or self.height(r)
        qs = [q for q in self.queries if q != r and self.S[q] >= y - x]
        for i in range(k):
            q = qs[i % len(qs)]
            self.rows.append((q, r, int(self.B[q]), int(self.B[q] + y - x), x, y, 0))

    def dovetail(self, r, x, y):
        """a sensitive record on [x, y) (trimmed) of target r that the oracle types kAB / kBA after trim; x == 0: a query's
        suffix on the target's prefix, y == span: a query's prefix on its suffix, else the longer overhang decides"""
        n = y - x
        o = self.front.o
        for q in self.queries:
            if q == r or self.S[q] < n + 600:
                continue
            for a0 in (int(self.E[q]) - n, int(self.B[q])):
                c = [a0, a0 + n, x + int(self.B[r]), y + int(self.B[r]), n]
                ok, c2, t = o.overlap_trim_type(q, r, 0, c)
                if ok and t in (3, 4) and (int(c2[2]), int(c2[3])) == (x + self.B[r], y + self.B[r]):
                    self.rows.append((q, r, a0, a0 + n, x, y, 0))
                    return True
        return False

    def take(self, r, role, plateaus):
        assert r not in self.used and len(self.used) < kMaxTargets
        self.used.append(r)
        self.roles[r] = role
        for p in plateaus:
            self.stack(r, *p)

    def free(self, stacks=1):
        """candidates not taken yet; with self.want set, those that one stack leaves in that tier (stacks = 0: all)"""
        out = [r for r in self.candidates if r not in self.used and r not in self.partners]
        if self.want and stacks:
            out = [r for r in out if tier(int(self.ds.read_len[r]), int(self.base_events[r]) + 2 * self.height(r) + 2) == self.want]
        return out

    # -- roles; each returns the target it took, or None
    def inner(self, role="inner plateau", edge=None):
        """a plateau over [0.35, 0.55) of the region; edge 'first' / 'second': moved until the hill's begin is the first
        position that is not left / its end the last that is not right"""
        for r in self.free():
            S, B = int(self.S[r]), int(self.B[r])
            x, y = int(0.35 * S), int(0.55 * S)
            if edge == "first":
                got = self.place(r, int(0.1 * S) + kUp, y, first=math.ceil(0.1 * S + B))
            elif edge == "second":
                got = self.place(r, x, int(0.9 * S) - kDown, second=math.floor(0.9 * S + B))
            else:
                got = self.place(r, x, y)
            if got:
                self.take(r, role, [got[:2]])
                return r
        return None

    def pair(self, accepted):
        """two plateaus, the floor between them: the outer pair has 2 w valid points of 2 w + g + 1, 0.9 of them while
        g <= 0.222 w - 1; accepted: a gap of 400 between plateaus of 0.15 of the region"""
        for r in self.free():
            S = int(self.S[r])
            w, g = (int(0.15 * S), 400) if accepted else (int(0.2 * S), int(0.25 * S))
            x = int(0.08 * S)
            if x + 2 * w + g + kWindow > int(0.9 * S):
                continue
            p = [(x, x + w), (x + w + g, x + 2 * w + g)]
            c = self.look(r, p)
            n_passed = sum(1 for d in c.log if d[:2] == (SHARE, "passed"))
            n_refused = sum(1 for d in c.log if d[:2] == (SHARE, "refused"))
            if (len(c.hills) == 1 and n_passed >= 3) if accepted else (len(c.hills) == 2 and n_refused >= 1):
                self.take(r, "two plateaus, the outer pair %s" % ("accepted" if accepted else "refused"), p)
                return r
        return None

    def left(self, version, side=None, fuzz=None):
        """a left hill.  version: 'bridged' (a designed dovetail ends at hill.second + 420; side / fuzz: a primary overlap with
        the target on that side ends at hill.second + fuzz; generated dovetails bridge it as well), 'exact' (the same dovetail
        on a hill that no generated one bridges), 'short' (that dovetail one base shorter), 'tie' (front == back), 'near tie' (front == back - 1: bridged)"""
        for r in self.free():
            S, B = int(self.S[r]), int(self.B[r])
            x = 400
            reach = max([e for b, e in self.generator_dovetails(r) if b - B < self.E[r] - e] + [0])
            if version == "bridged":
                ends = sorted((e, q) for b, e, q in self.primaries(r, side) if B + 2200 <= e <= B + int(0.45 * S))
                got = None
                for e, partner in ends:
                    got = self.place(r, x, e - fuzz - kDown - B, second=e - fuzz)
                    if got:
                        break
            else:
                # beyond the reach of every generated dovetail from the left
                y = max(reach - kFuzz - kDown - B + 2, int(0.3 * S))
                if y - x + kWindow > int(0.8 * S):
                    continue
                # (the one that only the designed dovetail bridges begins at the last position that is left)
                got = self.place(r, x, y) if version != "exact" else \
                    self.place(r, int(0.1 * S) + kUp, y + int(0.1 * S), first=math.ceil(0.1 * S + B) - 1)
            if not got:
                continue
            x, y, h = got
            if not h[0] < 0.1 * S + B or h[1] > 0.9 * S + B:
                continue
            if version == "bridged":
                ok = self.dovetail(r, 0, h[1] + kFuzz - B)
            elif version in ("short", "exact"):
                ok = h[1] + kFuzz > reach and self.dovetail(r, 0, h[1] + kFuzz - (1 if version == "short" else 0) - B)
            else:
                x0 = int(0.095 * S)
                ok = h[1] + kFuzz > reach and h[1] + kFuzz <= B + S - x0 - 1 and \
                    self.dovetail(r, x0, S - x0 - (1 if version == "near tie" else 0))
            if ok:
                if version == "bridged":
                    self.partners.add(partner)      # (a hill on the other read would decide about this overlap first, or as well)
                self.take(r, "left hill, %s%s" % (version, ", %s side at +%d" % (side, fuzz) if side else ""), [(x, y)])
                return r
        return None

    def right(self, version, side=None, fuzz=None, operand=None):
        """the mirror image: the designed dovetail begins at hill.first - 420, a primary overlap at hill.first - fuzz"""
        for r in self.free():
            S, B, E = int(self.S[r]), int(self.B[r]), int(self.E[r])
            y = S - 400
            reach = min([b for b, e in self.generator_dovetails(r) if b - B > E - e] + [E])
            if version == "bridged":
                begins = sorted(((b, q) for b, e, q in self.primaries(r, side) if B + int(0.55 * S) <= b <= E - 2200), reverse=True)
                got = None
                for b, partner in begins:
                    got = self.place(r, b + fuzz + kUp - B, y, first=b + fuzz)
                    if got:
                        break
            else:
                x = min(reach + kFuzz + kUp - B - 2, int(0.7 * S))
                if y - x + kWindow > int(0.8 * S):
                    continue
                # (... ends at the first position that is right)
                got = self.place(r, x, y) if version != "exact" else \
                    self.place(r, x - int(0.1 * S), int(0.9 * S) - kDown, second=math.floor(0.9 * S + B) + 1)
            if not got:
                continue
            x, y, h = got
            if not h[1] > 0.9 * S + B or h[0] < 0.1 * S + B:
                continue
            # (operand: the plateau is so long that it is the target's median; which of max(component median, p10) is larger)
            if operand and not any(d[:2] == (MAX_OPERAND, operand) and d[2] >= 5 for d in self.look(r, [(x, y)]).log):
                continue
            if version == "bridged":
                ok = self.dovetail(r, h[0] - kFuzz - B, S)
            elif version in ("short", "exact"):
                ok = h[0] - kFuzz < reach and self.dovetail(r, h[0] - kFuzz + (1 if version == "short" else 0) - B, S)
            else:
                x0 = int(0.095 * S)
                ok = h[0] - kFuzz < reach and h[0] - kFuzz >= B + x0 + 1 and \
                    self.dovetail(r, x0 + (1 if version == "near tie" else 0), S - x0)
            if ok:
                if version == "bridged":
                    self.partners.add(partner)
                self.take(r, "right hill, %s%s%s" % (version, ", %s side at -%d" % (side, fuzz) if side else "",
                                                     ", median above 1.42 * component median, the larger is p10" if operand else ""),
                          [(x, y)])
                return r
        return None

    def both(self):
        """one hill that begins in the first tenth and ends in the last: the plateau as long as the 0.84 rule lets it be"""
        for r in self.free():
            S, B = int(self.S[r]), int(self.B[r])
            w = int(0.84 * S) - kWindow - 4
            x = (S - w) // 2
            got = self.place(r, x, x + w)
            if got and got[2][0] < 0.1 * S + B and got[2][1] > 0.9 * S + B:
                self.take(r, "left and right at once", [got[:2]])
                return r
        return None

    def high_median(self, operand=None):
        """the plateau covers 0.6 of the region: the target's median is the plateau's height; operand 'p10' / 'dm': which
        of max(component median, p10) is the larger"""
        for r in self.free():
            S = int(self.S[r])
            got = self.place(r, int(0.2 * S), int(0.8 * S))
            if not got:
                continue
            c = self.look(r, [got[:2]])
            sides = dict(d[:2] for d in c.log)
            if sides.get(MEDIAN_SWITCH) == "taken" and operand in (None, sides.get(MAX_OPERAND)):
                self.take(r, "median above 1.42 * component median, the larger is %s" % sides[MAX_OPERAND], [got[:2]])
                return r
        return None

    def peak_end(self):
        """The peak test refuses a pair, and the larger of its two ends is w_first.  From left to right: 600 bases at + t,
        447 bases of the read's own coverage c, 399 bases at + m, then 2500 at + p, a quarter of c (no slope).  The first
        position at + p is a down region of its own: the + t stretch ends 847 bases back and is above 1.42 (c + p).  It pairs
        with the up region before the + m stretch, whose end lies at c: c + m is above 1.42 c and - m is the largest that does
        it - not above 1.42 (c + p).  The pairs that would cover the stretch have too few valid points: c and c + p are at or
        below uint32(1.42 * component median)."""
        for r in self.free(0):
            S, B = int(self.S[r]), int(self.B[r])
            row = self.base_row(r)
            for t0 in (int(0.15 * S), int(0.25 * S), int(0.35 * S), int(0.45 * S)):
                t1 = t0 + 600
                if t1 + 846 + 2500 + 900 > S:
                    continue
                near = row[B + t0 - 900:B + t1 + 846 + 2500 + 900]
                cmin, cmax = int(near.min()), int(near.max())
                p = int(0.25 * cmin)
                t = int(0.42 * cmax + 1.42 * p) + 6
                if tier(int(self.ds.read_len[r]), int(self.base_events[r]) + 2 * (t + t + p)) != self.want:
                    continue
                for m in range(int(0.42 * cmax + 1.42 * p) + 2, int(0.42 * cmin), -1):
                    stacks = [(t0, t1, t), (t1 + 447, t1 + 846, m), (t1 + 846, t1 + 846 + 2500, p)]
                    c = self.look(r, stacks)
                    if (PEAK, "none") not in [d[:2] for d in c.log]:
                        continue
                    TWEAK["peak end"] = True
                    try:
                        wrong = self.look(r, stacks).hills
                    finally:
                        TWEAK.clear()
                    if wrong != c.hills:
                        self.take(r, "the peak test refuses a pair whose larger end is w_first", stacks)
                        return r
                    break
        return None

    def smallest_component(self):
        size = self.st["comp_size"]
        free = self.free()
        if not free:
            return None
        small = min(size[r] for r in free)
        for r in free:
            if size[r] != small:
                continue
            S = int(self.S[r])
            got = self.place(r, int(0.35 * S), int(0.55 * S))
            if got:
                self.take(r, "plateau in the smallest component (%d reads)" % small, [got[:2]])
                return r
        return None

    def sensitive(self):
        return concat(self.gen, records(self.rows)) if self.rows else self.gen


def _design(name):
    b = Builder(name)
    if name == "position":
        # (its eight reads are one component: plateaus over more than half of a read on at most three of them, or the
        # component's median is a plateau's height)
        plan = [b.smallest_component, lambda: b.inner("inner plateau, first at the left edge", "first"),
                lambda: b.inner("inner plateau, second at the right edge", "second"), lambda: b.pair(True), lambda: b.pair(False),
                b.both, b.high_median]
    elif name == "cap2048":
        plan = [lambda s=s, z=z: b.left("bridged", s, z) for s in "ab" for z in (419, 420)] + \
               [lambda s=s, z=z: b.right("bridged", s, z) for s in "ab" for z in (419, 420)]
    else:
        plan = [("cap 1024", b.peak_end), ("cap 512", lambda: b.left("exact")), ("cap 1024", lambda: b.left("short")),
                ("cap 512", lambda: b.left("tie")), ("cap 1024", lambda: b.left("near tie")), ("cap 1024", lambda: b.right("exact")),
                ("cap 512", lambda: b.right("short")), ("cap 1024", lambda: b.right("tie", operand="p10"))]
    b.missed = []
    for k, step in enumerate(plan):
        b.want, step = step if isinstance(step, tuple) else (None, step)
        if step() is None:
            b.missed.append(k)
    return b


class CaseSet:
    """a base set, its sensitive set with the designed records, the oracle's results and the model's trace"""

    def __init__(self, name):
        b = _design(name)
        self.name, self.ds, self.sens, self.targets, self.roles, self.missed = name, b.ds, b.sensitive(), b.used, b.roles, b.missed
        self.n_designed = len(b.rows)
        ev = events(self.ds, self.sens)
        self.tiers = {r: tier(int(self.ds.read_len[r]), int(ev[r])) for r in self.targets}
        self.st, self.trace = sensitive_pass(self.ds, self.sens)
        o = self.st["oracle"]
        self.st["data"] = {r: o.pile_data(r) for r in self.targets}
        o.build_graph()
        self.st["n_tr"] = o.remove_transitive_edges()
        self.st["edges"] = o.edges()


_sets = {}


def case_set(name):
    """built once per process, never changed"""
    if name not in _sets:
        _sets[name] = CaseSet(name)
    return _sets[name]
