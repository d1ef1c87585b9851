"""Crafted reads and overlap lists whose containment removal runs deep: chains, nested reads, rings, and the tail's two scans.

Graph::construct deletes contained reads in file order (reference graph.cpp:464-483): a record of type kB deletes its query, one of
type kA its target, unless the other read - the record's KEEPER - was deleted earlier in the file, or (second pass only) has a
chimeric region.  The tail does it twice more without that guard, over the overlaps (class 0) and then over the internals
(class 1) (:831-866).  A case here is
  read lengths | an overlap list (grouped by query, no (a, b) twice in a run) | per read ONE coverage row, flat with at most one dip
and the bookkeeping of the design: for every record that is meant to delete a read its (stage, file position, target, keeper,
type), per chain its depth, and a describe() for failure messages.  model() is the Jacobi iteration of
  X[t] = min(base[t], min{key_i : target_i = t, X[keeper_i] > key_i}),   key = position in the file
over the designed killers of one stage: what any solver of that fixed point has to find, and how many rounds the plain iteration
takes - the longest chain of killers, plus the round that sees nothing move.

Geometry.  Pass-2 chains: r_k lies whole on r_(k-1) with `front` bases of the container before it and `back` behind it; as a kB
record the contained read is the query, as a kA record the target (front + back >= 1, or Overlap::type says kB).  Reverse-strand
records carry the target's coordinates on its forward strand, the way the file has them; Overlap::type mirrors them (overlap.cpp:
211-216).  The `mirror` chains are built so that the mirrored coordinates say kB and the unmirrored ones kAB.
Guarded chains (class 0): the same, every read at kValue with a dip to kShallow - a pit under find_slopes(1.82), not chimeric at
the component's median kValue: every keeper is guarded in the second pass, every record is kept, and the tail's first scan runs
the chain.  Internal chains (class 1): reads of 3 000 bases with a dip to kDeep at 1550, prefix on prefix (kX while the reads are
whole), and a hub whose suffix lies on every read's prefix so that they are members of a component; broken, every read keeps
[0, 1550), the records are kB, and the tail's second scan runs the chain.

Plain Python and numpy; nothing here touches a device or the oracle.
"""
import numpy as np

from rala_amd.synth import Overlaps

KX, KA, KB, KAB, KBA = range(5)
PASS2, TAIL0, TAIL1 = 0, 1, 2
STAGE_NAMES = ("pass 2", "tail class 0", "tail class 1")
INF = np.iinfo(np.int64).max

kValue = 300           # every row's level, and so every pile's and every component's median
kShallow = 164         # a dip that is a pit (300 > int(164 * 1.82)) and not chimeric at 300 (164 * 1.84 > 300)
kDeep = 100            # a dip that is chimeric at 300
kPitWidth = 3
kPitAt = 700           # a guard's pit
kBreakAt = 1550        # the pit an internal chain's reads are broken over: [0, 1550) is the longer side of 3 000
kLong = 3000
kShort = 1300          # the shortest read (Pile::shrink wants 1 260, pile.cpp:307)

assert kValue > int(kShallow * 1.82) and not kShallow * 1.84 <= kValue and kDeep * 1.84 <= kValue


def overlap_type(a_len, a_begin, a_end, b_len, b_begin, b_end, strand, mirror=True):
    """Overlap::type (overlap.cpp:194-259) of a record between two whole reads; mirror = False: what a reader that forgot to
    mirror a reverse-strand target's coordinates would say"""
    if strand and mirror:
        b_begin, b_end = b_len - b_end, b_len - b_begin
    a_tail, b_tail = a_len - a_end, b_len - b_end
    overhang = min(a_begin, b_begin) + min(a_tail, b_tail)
    if a_end - a_begin < (a_end - a_begin + overhang) * 0.875 or b_end - b_begin < (b_end - b_begin + overhang) * 0.875:
        return KX
    if a_begin <= b_begin and a_tail <= b_tail:
        return KB
    if a_begin >= b_begin and a_tail >= b_tail:
        return KA
    if abs((a_end - a_begin) - (b_end - b_begin)) < max(a_end - a_begin, b_end - b_begin) * 0.01:
        ext = int(0.05 * max(a_len, b_len))
        if abs(a_begin - b_begin) < ext:
            return KA if a_tail >= b_tail else KB
        if abs(a_tail - b_tail) < ext:
            return KA if a_begin >= b_begin else KB
    return KAB if a_begin > b_begin else KBA


class Case:
    pass


class Chain:
    """depth: the longest chain of designed killers in it, each one's keeper the next one's target in file order - what the
    fixed point's rounds have to reach; levels: its reads but one"""

    def __init__(self, name, stage, depth, levels=None):
        self.name, self.stage, self.depth, self.levels = name, stage, depth, depth if levels is None else levels
        self.reads = []         # labels while building, ids in the case: the top container first
        self.targets = []       # the reads some designed killer targets


class Builder:
    """reads get labels; ids are dealt out at the end, one per group in turn: every group's ids ascend in the order it lists its
    reads, and the groups are interleaved in id space"""

    def __init__(self, name):
        self.name = name
        self.length, self.pit, self.role = [], {}, {}
        self.groups, self.records, self.killers, self.chains, self.bystanders = [], [], [], [], []

    def read(self, length, pit=None, role=""):
        self.length.append(int(length))
        r = len(self.length) - 1
        if pit is not None:
            assert pit[0] + kPitWidth < length
            self.pit[r] = pit
        self.role[r] = role
        return r

    def group(self, labels):
        self.groups.append(list(labels))

    def record(self, a, b, a_begin, a_end, b_begin, b_end, strand=0):
        assert 0 <= a_begin < a_end <= self.length[a] and 0 <= b_begin < b_end <= self.length[b], (a, b)
        self.records.append((a, b, a_begin, a_end, b_begin, b_end, strand))
        return len(self.records) - 1

    def killer(self, stage, rec, target, keeper, typ):
        assert {target, keeper} == set(self.records[rec][:2])
        self.killers.append((stage, rec, target, keeper, typ))

    def contain(self, stage, inner, outer, front, kind, strand=0):
        """`inner` whole on `outer`, `front` bases of outer before it (as Overlap::type sees it); kind KB: inner is the query"""
        li, lo = self.length[inner], self.length[outer]
        assert front + li <= lo
        if kind == KB:
            b0 = lo - front - li if strand else front
            rec = self.record(inner, outer, 0, li, b0, b0 + li, strand)
        else:
            rec = self.record(outer, inner, front, front + li, 0, li, strand)
        self.killer(stage, rec, inner, outer, kind)
        return rec

    # ---- the designs ----------------------------------------------------------------------------------------------------------
    def chain(self, name, depth, kinds, front, back, strand=0, stage=PASS2, pit=None, descending=False, bottom=kShort):
        """depth + 1 reads; r_k on r_(k-1) by a record of kind kinds[k % len(kinds)]"""
        # (descending ids: every keeper's own killer comes later in the file - everybody below the top dies at once)
        c = Chain(name, stage, 1 if descending else depth, depth)
        for k in range(depth + 1):
            c.reads.append(self.read(bottom + (depth - k) * (front + back), pit, "%s, level %d of %d" % (name, k, depth)))
        for k in range(1, depth + 1):
            self.contain(stage, c.reads[k], c.reads[k - 1], front, kinds[k % len(kinds)], strand)
        c.targets = c.reads[1:]
        self.group(c.reads[::-1] if descending else c.reads)
        self.chains.append(c)
        return c

    def mirror_chain(self, name, depth):
        """reverse strand, r_k[100, len) on the last bases of r_(k-1) but 150 - in the file the target's first bases: kB mirrored,
        kAB read without mirroring"""
        c = Chain(name, PASS2, depth)
        for k in range(depth + 1):
            c.reads.append(self.read(kShort + 50 * (depth - k), None, "%s, level %d of %d" % (name, k, depth)))
        for k in range(1, depth + 1):
            a, b = c.reads[k], c.reads[k - 1]
            span = self.length[a] - 100
            assert self.length[b] == span + 150
            rec = self.record(a, b, 100, 100 + span, 0, span, 1)
            self.killer(PASS2, rec, a, b, KB)
        c.targets = c.reads[1:]
        self.group(c.reads)
        self.chains.append(c)
        return c

    def nested(self, name, depth, distances):
        """equal reads; r_k lies on r_(k-d) for every d of distances: that many killers per target, keepers of different fates.
        r_k survives iff none of its containers does: with distances 1 .. c every (c + 1)-th read survives; (1, 2, 4, 5, 7) has
        no multiple of 3, so every third one does"""
        period = 3 if distances == (1, 2, 4, 5, 7) else len(distances) + 1
        assert period == 3 or distances == tuple(range(1, len(distances) + 1))
        # (whether r_0 is there decides the phase of the whole pattern, and a round carries that at most max(distances) levels on)
        c = Chain(name, PASS2, depth // max(distances), depth)
        c.period = period
        c.reads = [self.read(kShort, None, "%s, level %d of %d" % (name, k, depth)) for k in range(depth + 1)]
        for k in range(1, depth + 1):
            for d in distances:
                if d <= k:
                    self.contain(PASS2, c.reads[k], c.reads[k - d], 0, KB)
        c.targets = c.reads[1:]
        c.containers = len(distances)
        self.group(c.reads)
        self.chains.append(c)
        return c

    def ring(self, name, n, rotate):
        """n equal reads, each whole on the next: a keeper cycle.  The file decides: the read whose run comes last survives.  Ids
        are rotated: the ring's first read in the file is its member `rotate`"""
        c = Chain(name, PASS2, 2, n - 1)
        c.reads = [self.read(kShort, None, "%s, member %d of %d" % (name, k, n)) for k in range(n)]
        for k in range(n):
            self.contain(PASS2, c.reads[k], c.reads[(k + 1) % n], 0, KB)
        c.targets = list(c.reads)
        self.group(c.reads[rotate:] + c.reads[:rotate])
        self.chains.append(c)
        return c

    def internal_chain(self, name, depth):
        c = Chain(name, TAIL1, depth)
        hub = self.read(kLong, None, "%s, the hub" % name)
        c.reads = [self.read(kLong, (kBreakAt, kDeep), "%s, level %d of %d" % (name, k, depth)) for k in range(depth + 1)]
        for r in c.reads:
            self.record(hub, r, kLong - 500, kLong, 0, 500)
        for k in range(1, depth + 1):
            rec = self.record(c.reads[k], c.reads[k - 1], 0, 1500, 0, 1500)
            self.killer(TAIL1, rec, c.reads[k], c.reads[k - 1], KB)
        c.targets = c.reads[1:]
        c.hub = hub
        self.group([hub] + c.reads)
        self.chains.append(c)
        return c

    def dovetails(self, n=40):
        """reads 700 bases apart on a line: suffix on prefix of the next and the next but one (kAB), the second one transitive"""
        rs = [self.read(2000, None, "bystander %d of %d: dovetails only" % (k, n)) for k in range(n)]
        for k in range(n):
            if k + 1 < n:
                self.record(rs[k], rs[k + 1], 700, 2000, 0, 1300)
            if k + 2 < n:
                self.record(rs[k], rs[k + 2], 1400, 2000, 0, 600)
        self.group(rs)
        self.bystanders = rs

    # ---- ids, the file, the bookkeeping ---------------------------------------------------------------------------------------
    def build(self):
        if not self.bystanders:
            self.dovetails()
        n = len(self.length)
        ident = np.full(n, -1, dtype=np.int64)
        at, nxt = [0] * len(self.groups), 0
        while nxt < n:
            for g, labels in enumerate(self.groups):
                if at[g] < len(labels):
                    assert ident[labels[at[g]]] < 0, "a read in two groups"
                    ident[labels[at[g]]] = nxt
                    at[g] += 1
                    nxt += 1
        assert (ident >= 0).all()
        rec = np.array(self.records, dtype=np.int64).reshape(-1, 7)
        a_id, b_id = ident[rec[:, 0]], ident[rec[:, 1]]
        order = np.argsort(a_id, kind="stable")             # grouped by query; a run keeps the order its records were added in
        where = np.empty(len(order), dtype=np.int64)
        where[order] = np.arange(len(order))
        a_id, b_id, rec = a_id[order], b_id[order], rec[order]
        assert len(np.unique(a_id * n + b_id)) == len(a_id) and (a_id != b_id).all(), "a pair twice in a run"
        span = np.maximum(rec[:, 3] - rec[:, 2], rec[:, 5] - rec[:, 4])
        case = Case()
        case.name = self.name
        case.n_reads = n
        case.read_len = np.zeros(n, dtype=np.uint32)
        case.read_len[ident] = self.length
        case.overlaps = Overlaps(a_id=a_id, b_id=b_id, a_begin=rec[:, 2], a_end=rec[:, 3], b_begin=rec[:, 4], b_end=rec[:, 5],
                                 length=span, strand=rec[:, 6].astype(np.uint8))
        case.pit = {int(ident[r]): p for r, p in self.pit.items()}
        case.role = {int(ident[r]): t for r, t in self.role.items()}
        k = np.array(self.killers, dtype=np.int64).reshape(-1, 5)
        by_pos = np.argsort(where[k[:, 1]], kind="stable")
        k = k[by_pos]
        case.k_stage, case.k_pos, case.k_target, case.k_keeper, case.k_type = (
            k[:, 0], where[k[:, 1]], ident[k[:, 2]], ident[k[:, 3]], k[:, 4])
        case.where = where                                  # builder's record number -> position in the file
        for c in self.chains:
            c.reads = [int(ident[r]) for r in c.reads]
            c.targets = [int(ident[r]) for r in c.targets]
            if hasattr(c, "hub"):
                c.hub = int(ident[c.hub])
        case.chains = self.chains
        case.bystanders = [int(ident[r]) for r in self.bystanders]
        case.ident = ident
        case.row_of = row_of                                # (parity.crafted_stages takes the rows from here)
        return case


def row_of(case, r):
    """the read's coverage row: flat at kValue, the dip where its pit is"""
    row = np.full(int(case.read_len[r]), kValue, dtype=np.uint16)
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
    """aux of rala_hip_get_intervals(0): the row's minimum over [first, second], both ends inclusive (pile.cpp:368-375)"""
    aux = np.zeros(len(pairs), dtype=np.uint32)
    for r in np.nonzero(offs[1:] > offs[:-1])[0]:
        row = row_of(case, int(r))
        for k in range(int(offs[r]), int(offs[r + 1])):
            aux[k] = row[int(pairs[k][0]):int(pairs[k][1]) + 1].min()
    return aux


def model(case, stage, valid, alive_before):
    """Jacobi iteration of X[t] = min(base[t], min{key_i : target_i = t, X[keeper_i] > key_i}) over the designed killers of
    `stage` whose record is valid, from X = base (0 for a read that is dead before the stage, never otherwise).
    Returns (died, rounds): the reads the stage deletes, and the rounds until nothing moves, that last round included."""
    pick = (case.k_stage == stage) & (np.asarray(valid)[case.k_pos] != 0)
    key, target, keeper = case.k_pos[pick], case.k_target[pick], case.k_keeper[pick]
    base = np.where(np.asarray(alive_before) != 0, INF, 0)
    x, rounds = base.copy(), 0
    while True:
        rounds += 1
        nxt = base.copy()
        fire = x[keeper] > key
        np.minimum.at(nxt, target[fire], key[fire])
        if (nxt == x).all():
            break
        x = nxt
        assert rounds <= len(key) + 2, "the iteration does not settle"
    return (x != INF) & (base == INF), rounds


def killers_of(case, r):
    return np.nonzero(case.k_target == r)[0]


def describe(case, r):
    """what the bookkeeping knows about read r, for a failure's message"""
    text = "read %d: %s" % (r, case.role.get(r, "?"))
    if r in case.pit:
        text += ", pit at %d down to %d" % case.pit[r]
    ks = killers_of(case, r)
    if len(ks):
        text += "; designed killers: " + ", ".join(
            "record %d (%s, %s, keeper %d)" % (case.k_pos[i], STAGE_NAMES[case.k_stage[i]], "kA" if case.k_type[i] == KA else "kB",
                                               case.k_keeper[i]) for i in ks[:6])
        if len(ks) > 6:
            text += " and %d more" % (len(ks) - 6)
    return text


# ---- the cases --------------------------------------------------------------------------------------------------------------
DEPTHS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 300)
DEEPEST = 1100                  # more rounds than the finish kernel has threads
_KINDS = {"kB": ((KB,), 0, 1), "kA": ((KA,), 1, 0), "alt": ((KB, KA), 1, 1)}


def _depths(name):
    b = Builder(name)
    plan = [(1, "kB", 0), (2, "kA", 0), (3, "alt", 0), (7, "kB", 0), (8, "kA", 1), (9, "alt", 0), (63, "kA", 0), (64, "alt", 1),
            (65, "kB", 1), (300, "kB", 0), (300, "kA", 0), (300, "alt", 0), (7, "alt", 1), (9, "kB", 1), (63, "kB", 0), (64, "kA", 0)]
    for depth, kind, strand in plan:
        kinds, front, back = _KINDS[kind]
        b.chain("%s%s_%d" % (kind, "_reverse" if strand else "", depth), depth, kinds, front, back, strand)
    for depth in (1, 2, 3):
        b.mirror_chain("mirror_%d" % depth, depth)
    b.chain("kB_%d" % DEEPEST, DEEPEST, (KB,), 0, 1)
    return b.build()


RINGS = (2, 3, 4, 64, 65, 257)


def _nested(name):
    b = Builder(name)
    b.nested("nested3_300", 300, (1, 2, 3))
    b.nested("nested5_300", 300, (1, 2, 4, 5, 7))
    b.chain("descending_300", 300, (KB,), 0, 1, descending=True)
    b.chain("descending_kA_9", 9, (KA,), 1, 0, descending=True)
    for n in RINGS:
        b.ring("ring_%d" % n, n, n // 3 + 1)
    return b.build()


MANY_CHAINS = 45


def _many(name):
    b = Builder(name)
    for k in range(MANY_CHAINS):
        b.chain("many%d_%d" % (k, 300 + k % 3), 300 + k % 3, (KB,), 0, 0)
    return b.build()


TAIL_DEPTHS = (1, 2, 65, 300)


def _guarded(name):
    b = Builder(name)
    for k, depth in enumerate(TAIL_DEPTHS):
        kinds, front, back = _KINDS[("kB", "kA", "alt", "kB")[k]]
        b.chain("guarded_%d" % depth, depth, kinds, front, back, stage=TAIL0, pit=(kPitAt, kShallow))
    return b.build()


def _internal(name):
    b = Builder(name)
    for depth in TAIL_DEPTHS:
        b.internal_chain("internal_%d" % depth, depth)
    return b.build()


# the crossed scenarios: name -> what flipping its one designed record (or dip) changes, checked in the oracle
FLIPS = {"class0_frees_class1": "drop the class-0 record: its target lives, and the class-1 target behind it dies",
         "guarded_keeper": "drop the guarded record: its target, deleted in the tail, lives; the read it kept in pass 2 is dead anyway",
         "broken_guard": "make the guard's pit shallow: the guard stays whole and the tail deletes the target"}


def _crossed(name, flip=None):
    assert flip is None or flip in FLIPS
    b = Builder(name)
    b.expect_alive, b.expect_dead, b.flipped = [], [], []
    long_pit, guard_pit = (kBreakAt, kDeep), (kPitAt, kShallow)

    # a class-1 killer whose keeper class 0 deletes (its target survives), and the twin without the class-0 record (it dies)
    hub = b.read(kLong, None, "class0_frees_class1: the hub")
    T, K = b.read(kLong, long_pit, "class0_frees_class1: T, class-1 target"), b.read(kLong, long_pit, "class0_frees_class1: K, its keeper")
    G = b.read(kLong + 20, guard_pit, "class0_frees_class1: G, contains K, guarded")
    T2, K2 = b.read(kLong, long_pit, "class0_frees_class1: twin T'"), b.read(kLong, long_pit, "class0_frees_class1: twin K'")
    for r in (T, K, T2, K2):
        b.record(hub, r, kLong - 500, kLong, 0, 500)
    b.killer(TAIL1, b.record(T, K, 0, 1500, 0, 1500), T, K, KB)
    b.killer(TAIL1, b.record(T2, K2, 0, 1500, 0, 1500), T2, K2, KB)
    if flip != "class0_frees_class1":
        b.contain(TAIL0, K, G, 10, KB)
        b.expect_alive += [hub, T, G, K2]
        b.expect_dead += [K, T2]
    else:
        b.flipped = [K, T]
    b.group([hub, G, K, T, K2, T2])

    # a pass-2 killer whose keeper is guarded (so it is alive in pass 2 and dies in the tail) beside one whose keeper is not
    A = b.read(kShort + 40, guard_pit, "guarded_keeper: A, guarded")
    B, C = b.read(kShort + 20, None, "guarded_keeper: B, on A"), b.read(kShort, None, "guarded_keeper: C, on B")
    A2, B2, C2 = (b.read(kShort + 40 - 20 * k, None, "guarded_keeper: twin %s, nobody guarded" % "ABC"[k]) for k in range(3))
    if flip != "guarded_keeper":
        b.contain(TAIL0, B, A, 10, KB)
        b.expect_dead += [B]
    else:
        b.flipped = [B]
    b.contain(PASS2, C, B, 10, KB)
    b.contain(PASS2, B2, A2, 10, KB)
    b.contain(PASS2, C2, B2, 10, KB)
    b.expect_alive += [A, A2, C2]
    b.expect_dead += [C, B2]
    b.group([A, B, C])
    b.group([A2, B2, C2])

    # a guarded keeper whose pit IS chimeric: broken, it keeps [0, 1550), the record's part on it is [400, 1550) and the record
    # a dovetail (kBA) - no killer in the tail; its twin's pit is shallow, the twin stays whole and the tail deletes the target
    shallow = flip == "broken_guard"
    P = b.read(kLong, (kBreakAt, kShallow if shallow else kDeep), "broken_guard: P, guarded, its pit chimeric")
    Q = b.read(kShort, None, "broken_guard: Q, on P[400, 1700)")
    rec = b.record(Q, P, 0, kShort, 400, 400 + kShort)
    b.retyped = None if shallow else rec
    if shallow:
        b.killer(TAIL0, rec, Q, P, KB)
        b.flipped = [Q]
    else:
        b.expect_alive += [P, Q]
    P2 = b.read(kLong, (kBreakAt, kShallow), "broken_guard: twin P', guarded, its pit not chimeric")
    Q2 = b.read(kShort, None, "broken_guard: twin Q'")
    b.contain(TAIL0, Q2, P2, 400, KB)
    b.expect_alive += [P2]
    b.expect_dead += [Q2]
    b.group([P, Q])
    b.group([P2, Q2])

    case = b.build()
    case.expect_alive = [int(case.ident[r]) for r in b.expect_alive]
    case.expect_dead = [int(case.ident[r]) for r in b.expect_dead]
    case.flipped = sorted(int(case.ident[r]) for r in b.flipped)
    case.retyped = None if b.retyped is None else int(case.where[b.retyped])
    return case


def crossed_flipped(flip):
    """the crossed case with one scenario's designed record (or dip) flipped; same reads, same ids"""
    return _crossed("crossed~" + flip, flip)


CASES = {
    "depths": _depths,
    "nested_rings": _nested,
    "many": _many,
    "guarded": _guarded,
    "internal": _internal,
    "crossed": _crossed,
}
PASS2_CASES = ("depths", "nested_rings", "many")
TAIL_CASES = ("guarded", "internal", "crossed")

_built = {}


def case(name):
    """the named case, built once (it is never changed)"""
    if name not in _built:
        _built[name] = CASES[name](name)
    return _built[name]
