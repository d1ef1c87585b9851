"""Crafted per-read state and overlap lists that make every connected component's median observable.

The chimera stage gives every read the element at size / 2 of its component's sorted pile medians (reference graph.cpp:777-783) and
breaks the read over a pit whose minimum coverage `a` satisfies (double)a * 1.84 <= that median (pile.cpp:366-402).  A case here is
  read lengths | an overlap list (grouped by query, no (a, b) twice in a run) | per read ONE coverage row with begin = 0, end = length
and the bookkeeping that says which component every read was designed into, the component's designed median M and its probes:
  lower probe   a read whose pit has minimum a       - broken at M, not at M - 1
  upper probe   a read whose pit has minimum a + 1   - not broken at M, broken at M + 1
M is usable when such an `a` exists (checked with the predicate itself, in double).  A component median that is wrong by any amount in
either direction flips the begin / end of one of the two.  The probes' own row values are members of the component like any other.

Geometry: reads of about 2 kb; every overlap a same-strand dovetail of kSpan bases, a's suffix on b's prefix (kAB whatever the two
valid regions are shrunk to below); a row is flat at the value that is to be the pile's median, with at most one dip of kPitWidth
bases.  A probe has overlaps on one side only and its pit on the other one, so breaking it costs no overlap: a probe that is a query
only keeps [pit end, length), one that is a target only keeps [0, pit begin).  Only the bridge of the splitting component loses
overlaps, on purpose.

Plain Python and numpy; nothing here touches a device or the oracle.
"""
import numpy as np

from rala_amd.synth import Overlaps

kSpan = 500            # bases of every overlap (Overlap::trim wants 84 left, overlap.cpp:176)
kPitWidth = 3
kPitFront = 200        # a query-only probe's pit: [200, 202]
kPitBack = 203         # a target-only probe's pit: [length - 203, length - 201]
kPitBridge = 600       # the bridge's pit lies behind the overlaps on its prefix: they die with it
kLoose = 50            # row value of a live read without overlaps

LOW = "low"
HIGH = "high"


def chimeric(a, m):
    """the predicate of Pile::break_over_chimeric_pits (pile.cpp:370) for a pit of minimum a under median m"""
    return float(a) * 1.84 <= m


def probe_minimum(M):
    """a such that a pit of minimum a is broken at M and not at M - 1 and one of minimum a + 1 is not broken at M but at M + 1;
    None when M has no such a (M is not usable)"""
    guess = int(M / 1.84)
    for a in (guess - 1, guess, guess + 1):
        if a >= 4 and chimeric(a, M) and not chimeric(a, M - 1) and not chimeric(a + 1, M) and chimeric(a + 1, M + 1):
            return a
    return None


def usable_medians(lo, hi):
    return [M for M in range(lo, hi) if probe_minimum(M) is not None]


def detectable(value, dip):
    """Pile::find_slopes(1.82) flags the dip of a flat row: the window's maximum exceeds int(dip * 1.82) (pile.cpp:94-95)"""
    return value > int(dip * 1.82)


LOW_MEDIANS = usable_medians(12, 31)            # 12, 23
HIGH_MEDIANS = usable_medians(300, 1200)


# ---- value profiles: s pile medians (any order) whose element at s // 2 is M ------------------------------------------------------
def spread(s, M):
    """below and above M by at least three: in an even-sized component sorted[s / 2 - 1] is far more than a probe's step away"""
    if s == 2:
        return [M, M]
    k = s // 2
    return [M - 3 - (i % 3) for i in range(k)] + [M] + [M + 3 + (i % 5) for i in range(s - k - 1)]


def tied(s, M):
    """the selected value occurs in all places from s / 2 on but the last"""
    k = s // 2
    return [M - 4] * k + [M] * (s - k - 1) + [M + 5]


def equal(s, M):
    return [M] * s


def distinct(s, M):
    return list(range(M - s // 2, M - s // 2 + s))


# ---- shapes: overlaps (i, j) = member i's suffix on member j's prefix, over the positions of `core` in `ids` ------------------------
def chain(core, ids, rng):
    c = sorted(core, key=lambda m: ids[m])
    return list(zip(c[:-1], c[1:]))


def chain_permuted(core, ids, rng):
    c = [core[i] for i in rng.permutation(len(core))]
    return list(zip(c[:-1], c[1:]))


def star(core, ids, rng):
    hub = max(core, key=lambda m: ids[m])
    return [(m, hub) for m in core if m != hub]


def cliques(core, ids, rng):
    c = [core[i] for i in rng.permutation(len(core))]
    halves = (c[:len(c) // 2], c[len(c) // 2:])
    out = []
    for h in halves:
        out += [(h[i], h[j]) for i in range(len(h)) for j in range(i + 1, len(h))]
    if halves[0]:
        out.append((halves[0][-1], halves[1][-1]))        # the one overlap between them (neither has a run of its own otherwise)
    return out


def third(core, ids, rng):
    """clusters (x, y, z): x -> y, x -> z, and only x's THIRD overlap reaches the next cluster; y and z are queries of nothing"""
    c = [core[i] for i in rng.permutation(len(core))]
    if len(c) < 6:
        return chain_permuted(core, ids, rng)
    n = len(c) // 3
    out = []
    for t in range(n):
        x, y, z = c[3 * t:3 * t + 3]
        out += [(x, y), (x, z)]
        if t + 1 < n:
            out.append((x, c[3 * (t + 1) + 1]))
    out += [(c[3 * (n - 1)], m) for m in c[3 * n:]]         # what is left over: fourth and fifth of the last run
    return out


class Component:
    """values: a list, or f(s, M) with M picked from the class (LOW / HIGH) the builder assigns; shape: one of the functions above"""

    def __init__(self, name, size, values, shape, klass=None):
        self.name, self.size, self.values, self.shape, self.klass = name, size, values, shape, klass
        self.members = None     # read ids, filled by the builder
        self.M = None
        self.probes = {}        # role -> read id
        self.tiers = []         # (name, read ids, median) of what the component splits into


class Case:
    pass


def _loose_kinds(n):
    """0 member, 1 live without overlaps, 2 dead: dead reads at fixed ids (read 0 among them), loose live ones at the ranks where a
    wavefront, a block of 256 and a block of 1024 begin (rank = live reads before it: rank != id)"""
    kind = np.zeros(n, dtype=np.uint8)
    kind[[i for i in (0, 2, 100, 300, 700, 1500, 3100) if i < n]] = 2
    kind[np.arange(37, n, 257)] = 2
    rank = np.cumsum(kind != 2) - 1
    live = kind != 2
    want = (rank % 64 == 0) & ((rank < 256) | (rank % 256 == 0)) | (rank % 211 == 5)
    kind[live & want] = 1
    return kind


class CaseBuilder:
    def __init__(self, name, interleaved=True, seed=1, loose=True):
        self.name, self.interleaved, self.seed, self.loose = name, interleaved, seed, loose
        self.comps = []

    def add(self, comp):
        self.comps.append(comp)
        return comp

    def build(self):
        rng = np.random.default_rng(self.seed)
        n_members = sum(c.size for c in self.comps)
        n = n_members
        while True:
            kind = _loose_kinds(n) if self.loose else np.zeros(n, dtype=np.uint8)
            slots = np.nonzero(kind == 0)[0]
            if len(slots) >= n_members:
                break
            n += n_members - len(slots)
        kind[slots[n_members:]] = 1
        slots = slots[:n_members]
        if self.interleaved:
            # every component's smallest id from the front, in the order they were added - that is the order of their stretches
            # in the select's value array - and all other ids dealt out by one permutation
            n_comps = len(self.comps)
            rest = slots[n_comps:][rng.permutation(n_members - n_comps)]
            at = 0
            for k, c in enumerate(self.comps):
                c.members = [int(slots[k])] + [int(x) for x in rest[at:at + c.size - 1]]
                at += c.size - 1
        else:
            at = 0
            for c in self.comps:
                c.members = [int(x) for x in slots[at:at + c.size]]
                at += c.size
        # neighbours in root order (a component's stretch of the select's value array follows its smallest rank's) alternate
        # between low and high medians; a component with values of its own counts as what its median is
        order = sorted(self.comps, key=lambda c: min(c.members))
        last, n_low, n_high = HIGH, 0, 0
        for c in order:
            if callable(c.values):
                klass = c.klass or (LOW if last == HIGH else HIGH)
                if klass == LOW and c.size == 2:
                    klass = HIGH            # (the pair's upper probe IS the median: only a high one makes its own pit visible)
                if klass == LOW:
                    M = LOW_MEDIANS[n_low % len(LOW_MEDIANS)]
                    n_low += 1
                else:
                    M = HIGH_MEDIANS[(7 * n_high) % len(HIGH_MEDIANS)]
                    n_high += 1
                c.values = [int(v) for v in c.values(c.size, M)]
                last = klass
            else:
                c.values = [int(v) for v in c.values]
                last = LOW if sorted(c.values)[c.size // 2] < 100 else HIGH
            assert len(c.values) == c.size, c.name

        read_len = (2000 + 16 * (np.arange(n) % 5)).astype(np.uint32)
        value = np.full(n, kLoose, dtype=np.int64)
        value[kind == 2] = 0
        pit = {}                    # read -> (first position, dip value)
        runs = {}                   # query -> targets, in run order
        comp_of = np.full(n, -1, dtype=np.int64)

        def link(a, b):
            runs.setdefault(a, []).append(b)

        for ci, c in enumerate(self.comps):
            ids = c.members
            comp_of[ids] = ci
            value[ids] = c.values
            c.M = sorted(c.values)[c.size // 2]
            a = probe_minimum(c.M)
            if a is None:
                raise ValueError("%s/%s: median %d is not usable" % (self.name, c.name, c.M))
            c.a = a
            if getattr(c, "custom", None):
                c.custom(self, c, link, pit, read_len)
                continue
            # the two largest values are the probes' own: their dips must show against them
            by_value = sorted(range(c.size), key=lambda m: (c.values[m], m))
            up, lo = by_value[-1], by_value[-2]
            if not (detectable(c.values[up], a + 1) and detectable(c.values[lo], a)):
                raise ValueError("%s/%s: a probe's dip would not be a pit (values %d, %d; minimum %d)" %
                                 (self.name, c.name, c.values[lo], c.values[up], a))
            c.probes = {"lower": ids[lo], "upper": ids[up]}
            core = [m for m in range(c.size) if m not in (lo, up)]
            if not core:
                link(ids[lo], ids[up])
                pit[ids[lo]] = (kPitFront, a)
                pit[ids[up]] = (int(read_len[ids[up]]) - kPitBack, a + 1)
                continue
            for i, j in c.shape(core, ids, rng):
                link(ids[i], ids[j])
            anchor = core[len(core) // 2]
            link(ids[lo], ids[anchor])
            link(ids[up], ids[anchor])
            pit[ids[lo]] = (kPitFront, a)
            pit[ids[up]] = (kPitFront, a + 1)

        # overlaps that lead to dead reads: first in their query's run, so they take a place among the two the sampled round sees
        dead = np.nonzero(kind == 2)[0]
        queries = sorted(q for q in runs if q not in pit)
        for k, d in enumerate(dead[1::2]):
            if queries:
                q = queries[(k * 7919) % len(queries)]
                if int(d) not in runs[q]:
                    runs[q].insert(0, int(d))

        a_id, b_id = [], []
        for q in sorted(runs):
            assert len(set(runs[q])) == len(runs[q]), "a pair twice in the run of read %d" % q
            a_id += [q] * len(runs[q])
            b_id += runs[q]
        a_id, b_id = np.array(a_id, dtype=np.int64), np.array(b_id, dtype=np.int64)
        pairs = np.minimum(a_id, b_id) * n + np.maximum(a_id, b_id)
        assert len(np.unique(pairs)) == len(pairs) and (a_id != b_id).all(), "a pair of reads overlaps twice"
        la = read_len[a_id].astype(np.int64)
        span = np.full(len(a_id), kSpan)
        ov = Overlaps(a_id=a_id, b_id=b_id, a_begin=la - kSpan, a_end=la, b_begin=0 * span, b_end=span, length=span,
                      strand=np.zeros(len(a_id), dtype=np.uint8))

        case = Case()
        case.name = self.name
        case.n_reads = n
        case.read_len = read_len
        case.overlaps = ov
        case.kind = kind
        case.value = value.astype(np.uint16)
        case.pit = pit
        case.comps = self.comps
        case.comp_of = comp_of
        return case


def row_of(case, r):
    """the read's coverage row: flat at its value, the dip where its pit is"""
    row = np.full(int(case.read_len[r]), case.value[r], dtype=np.uint16)
    if r in case.pit:
        at, dip = case.pit[r]
        row[at:at + kPitWidth] = dip
    return row


def designed_pits(case):
    """CSR (offsets, pairs) of the pits the rows were built to have: [first, second] = the dip"""
    offs = np.zeros(case.n_reads + 1, dtype=np.uint64)
    pairs = []
    for r in range(case.n_reads):
        if r in case.pit:
            at = case.pit[r][0]
            pairs.append((at, at + kPitWidth - 1))
        offs[r + 1] = len(pairs)
    return offs, np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def pit_minima(case, offs, pairs):
    """aux of rala_hip_get_intervals(0): the row's minimum over [first, second], both ends inclusive - the range the lambda of
    Pile::break_over_chimeric_pits walks (pile.cpp:368-375)"""
    aux = np.zeros(len(pairs), dtype=np.uint32)
    for r in np.nonzero(offs[1:] > offs[:-1])[0]:
        row = row_of(case, int(r))
        for k in range(int(offs[r]), int(offs[r + 1])):
            aux[k] = row[int(pairs[k][0]):int(pairs[k][1]) + 1].min()
    return aux


def describe(case, r):
    """what the bookkeeping knows about read r, for a failure's message"""
    if case.kind[r] == 2:
        return "read %d: dead by design" % r
    if case.kind[r] == 1:
        return "read %d: live, without overlaps" % r
    c = case.comps[int(case.comp_of[r])]
    role = [k for k, v in c.probes.items() if v == r]
    text = "read %d: component %s (%d reads, designed median %d, probe minimum %d)" % (r, c.name, c.size, c.M, c.a)
    for name, ids, M in c.tiers:
        if r in ids:
            text += ", after the split in %s (median %d)" % (name, M)
    if role:
        text += ", its %s probe (pit minimum %d)" % (role[0], case.pit[r][1])
    elif r in case.pit:
        text += ", pit minimum %d" % case.pit[r][1]
    return text


# ---- the splitting component --------------------------------------------------------------------------------------------------
def _split_component():
    """17 reads around a bridge: eight on its prefix, eight behind its suffix.  All together have median M; the bridge's pit is
    chimeric under M, the bridge keeps its back and the overlaps on its prefix die: the left half (median M1 > M) and the right
    half with the bridge (M2 < M) are components of their own in the second round.  Probes: lower and upper for M (the upper one in
    the right half: M2 keeps it whole), and for M1 a second tier in the left half - neither is chimeric under M."""
    hi = HIGH_MEDIANS
    M2, M, M1 = hi[3], hi[5], hi[8]
    assert M2 + 8 < M and M + 8 < M1
    #       0..7 left: l0 .. l5 chain, 6 = second-tier lower, 7 = second-tier upper
    left = [M - 3, M - 3, M - 3, M1 - 3, M1, M1 + 3, M1 + 4, M1 + 5]
    #       8 bridge, 9..13 chain, 14 = lower probe for M, 15 = upper probe for M, 16 chain
    right = [M + 3, M2 - 4, M2 - 4, M2 - 4, M2 - 4, M2, M, M + 4, M]
    c = Component("split", 17, left + right, None)

    def custom(builder, c, link, pit, read_len):
        ids = c.members
        a, a1 = c.a, probe_minimum(M1)
        assert sorted(left)[4] == M1 and sorted(right)[4] == M2 and a1 is not None and not chimeric(a1, c.M)
        for i in range(5):
            link(ids[i], ids[i + 1])                    # l0 -> .. -> l5
        link(ids[5], ids[8])                            # l5's suffix on the bridge's prefix
        link(ids[6], ids[2])
        link(ids[7], ids[3])
        for i, j in ((8, 9), (9, 10), (10, 11), (11, 12), (12, 13), (13, 16), (14, 10), (15, 11)):
            link(ids[i], ids[j])
        pit[ids[8]] = (kPitBridge, a - 2)
        pit[ids[14]] = (kPitFront, a)
        pit[ids[15]] = (kPitFront, a + 1)
        pit[ids[6]] = (kPitFront, a1)
        pit[ids[7]] = (kPitFront, a1 + 1)
        for m in (8, 14, 15, 6, 7):
            assert detectable(c.values[m], pit[ids[m]][1])
        c.probes = {"lower": ids[14], "upper": ids[15], "second-tier lower": ids[6], "second-tier upper": ids[7], "bridge": ids[8]}
        c.tiers = [("the left half", ids[:8], M1), ("the right half", ids[8:], M2)]

    c.custom = custom
    return c


# ---- the cases ----------------------------------------------------------------------------------------------------------------
SIZES = (2, 3, 63, 64, 65, 66, 255, 256, 257, 1023, 1024, 1025)
_SHAPES = (chain, chain_permuted, star, cliques, third)


def _sizes(name, interleaved):
    b = CaseBuilder(name, interleaved=interleaved, seed=11)
    shapes = (chain_permuted, third, chain, star)
    # three of every size: that puts the stretches' starts on every residue mod 8 (asserted in the CPU test)
    for rep in range(3):
        for k, s in enumerate(SIZES):
            b.add(Component("size%d_%d" % (s, rep), s, spread, shapes[(k + rep) % 4]))
    return b.build()


def _high_byte(name):
    b = CaseBuilder(name, seed=5)
    lo0, hi1 = 253, 264                 # usable medians on either side of 256
    assert probe_minimum(lo0) is not None and probe_minimum(hi1) is not None
    big = [M for M in usable_medians(4200, 4400)][0]
    for s in (100, 101, 640):
        k = s // 2
        # the selected element is the LAST value with high byte 0: everything above it has high byte 1
        b.add(Component("last_of_byte0_%d" % s, s, [240 + (i % 10) for i in range(k)] + [lo0] + [256 + (i % 3) for i in range(s - k - 1)],
                        chain_permuted))
        # ... the FIRST with high byte 1: everything below it has high byte 0, up to 255
        b.add(Component("first_of_byte1_%d" % s, s, [255 - (i % 4) for i in range(k)] + [hi1] + [hi1 + (i % 300) for i in range(s - k - 1)],
                        chain_permuted))
    b.add(Component("all_equal_130", 130, equal, chain_permuted, HIGH))
    b.add(Component("all_distinct_200", 200, distinct, chain_permuted, HIGH))
    b.add(Component("all_distinct_33", 33, distinct, star, HIGH))
    b.add(Component("above_4096", 90, spread(90, big), third))
    b.add(Component("across_4096", 300, [4000 + (i % 90) for i in range(150)] + [big] + [big + 256 * (i % 5) + i for i in range(149)],
                    chain_permuted))
    return b.build()


def _ties(name):
    b = CaseBuilder(name, seed=9)
    for s in (7, 40, 63, 64):
        b.add(Component("tied_%d" % s, s, tied, chain_permuted))
        b.add(Component("equal_%d" % s, s, equal, star, HIGH))
    b.add(Component("tied_65", 65, tied, chain_permuted))
    return b.build()


def _shape(name, shape):
    b = CaseBuilder(name, seed=3)
    for s in (5, 8, 64, 65, 300):
        b.add(Component("%s_%d" % (shape.__name__, s), s, spread, shape))
    return b.build()


def _split(name):
    b = CaseBuilder(name, seed=4)
    b.add(Component("before", 9, spread, chain, LOW))
    b.add(_split_component())
    b.add(Component("after", 70, spread, chain_permuted, LOW))
    return b.build()


def _large(name):
    b = CaseBuilder(name, seed=8)
    for k in range(150):
        b.add(Component("small%d" % k, 2 + k % 4, spread, chain_permuted))
    b.add(Component("large", 33_000, spread, chain_permuted, HIGH))
    for k in range(150, 300):
        b.add(Component("small%d" % k, 2 + k % 4, spread, star))
    return b.build()


CASES = {
    "sizes_interleaved": lambda n: _sizes(n, True),
    "sizes_contiguous": lambda n: _sizes(n, False),
    "high_byte": _high_byte,
    "ties": _ties,
    "shape_chain": lambda n: _shape(n, chain),
    "shape_chain_permuted": lambda n: _shape(n, chain_permuted),
    "shape_star": lambda n: _shape(n, star),
    "shape_cliques": lambda n: _shape(n, cliques),
    "shape_third": lambda n: _shape(n, third),
    "split": _split,
    "large": _large,
}
LARGE = "large"

_built = {}


def case(name):
    """the named case, built once (it is never changed)"""
    if name not in _built:
        _built[name] = CASES[name](name)
    return _built[name]
