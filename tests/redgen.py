"""Seeded read sets built to sit ON the list limits of the reduce phase (kernels_reduce.inc, the reduce_* stages of sage2ov_device.hip).  The reads are
error free and made of planted sequences, so the generator -- not the statistics of a genome -- decides how long every list is, which form of the phase runs and what
the marks remove.  tests/test_redgen_host.py proves with the oracle alone that every case has the property it is named after; tests/test_gpu_reduce_limits.py compares
the device with the oracle and with `Case.model()`.

The gadgets (all reads of a case have one length L; rho = k + 20 bases of shared sequence make an overlap; every other part is random, so gadgets do not touch):

  fan        a hub H = X.R and c reads B = R[t:].Y (t = the read's offset, distinct random Y).  H overlaps every B, the B do not overlap each other, nothing precedes X
             or follows a Y: all c + 1 reads are unresolved and H's list has exactly c entries.  One offset holds at most 99 reads (its prefix key's bucket stays
             visible, hashTable.cpp:111-123); up to three offsets give lists of up to CONN_LIMIT entries.  All entries of one offset have the same overlap length: the
             order within them is by id and type (:853-871).
  stem       a second hub in front of the fan, Ha = S[0:L], Hb = S[s:L+s] with R = the end of S: Ha overlaps Hb and every B (by s bases less).  Both hubs' lists have
             c + 1 entries; Ha -> Hb -> B is a triangle, so Ha's marks remove its c entries to the B, and every B's marks remove its entry to Ha.
  blind fan  c >= 100 reads at one offset: the key is hidden, H sees no B while every B sees H through H's suffix key (one-sided discovery: the ranked form).  An edge
             then exists iff the read that sees the other is explored first (economyGraph.cpp:605), so every B must be explored before H is.  The serial search
             (:513-564) explores a read's neighbours before it marks the read: a root G0 = U.Z with the lowest id of the gadget, its neighbours Gj = Tj.Vj.U, and the
             B = R.M.Tj in groups of at most 99 per Gj are explored in that order -- root, the Gj, all B (each inserting its edge to the still unexplored H) -- and
             H only afterwards.  H's list consists of twins only, c of them: any length.  Its potential list (own hits + twins) has c entries too.
  isolated   a random read: unresolved, empty list.            chain   a tiling of a random sequence: resolved reads between two unresolved ends (candidates of the
                                                                       reciprocal pass in the lists).

The model (`Case.model()`) states, from the construction alone, what Context.reduce_stats() must report.  The short cut's two counters are part of it for the pure fans
only (a B's one-entry list settles with one list read; the hub reads a list per entry and gives up at the 25th).  With a finished oracle (`Case.model(oracle)`) the model
restates the serial search, its marks and the short cut on the reads' strings (`Walk`): list lengths and marked entries of every read are then held against
Oracle.export_mark_lengths, and the short cut's counters are known for every case -- which is what the two cases built by search need (sc_dup, sc_early).
There is no case for a read whose own list eliminates it (ra_shortcut: "a self edge"): no legal input has one -- the initial pass tests read2 != i (economyGraph.cpp:94),
explore() skips the read it explores because its status is already 1 (:605) -- so a list never names its own read."""
import numpy as np

CONN_LIMIT = 300                 # connections beyond which a read leaves the unresolved set (economyGraph.cpp:443)
LONG_BUCKET = 100                # entries from which a bucket is hidden (hashTable.cpp:111-123)
RA_FIRST, RA_CAP, RR_CAP = 128, 512, 1024      # kernels_reduce.inc: first size class of the marks, the LDS kernel's longest list, the device sort of potential lists
RA_SHORTCUT_LISTS = 24
FEW_MAX_THIRD = 1024             # unresolved reads up to which the replay route collects with k_red_collect_few
DEVICE_REDUCE_MIN = 4096         # unresolved reads from which the library takes a device form unasked
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canonical(s):
    r = revcomp(s)
    return s if s < r else r


def rnd(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


class Gadget:
    """reads + what the construction fixes: unresolved reads, list lengths of the unresolved reads with a non-empty list, potential-list lengths (blind fans),
    removed entries (None: left to the oracle), short-cut counters (None: not modelled)"""
    def __init__(self, reads, unresolved=None, lists=(), removed=0, potential=(), shortcut=None, hidden=False):
        self.reads, self.unresolved, self.lists, self.removed, self.potential, self.shortcut, self.hidden = list(reads), unresolved, list(lists), removed, list(potential), shortcut, hidden


def fan(rng, k, L, c, stem=False):
    """symmetric fan of c <= CONN_LIMIT - 1 reads over up to three offsets, with or without the stem"""
    rho, s = k + 20, 8
    per = [c // 3 + (1 if t < c % 3 else 0) for t in range(3)] if c >= LONG_BUCKET else [c]
    assert max(per, default=0) < LONG_BUCKET and c + (1 if stem else 0) <= CONN_LIMIT
    S = rnd(rng, L + s)
    R = S[L + s - rho:]
    hubs = [S[s:]] + ([S[:L]] if stem else [])
    bs = [R[t:] + rnd(rng, L - (rho - t)) for t, n in enumerate(per) for _ in range(n)]
    n = c + len(hubs)
    if not stem:
        if c == 0:
            return Gadget(hubs, 1, [], shortcut=(0, 0))
        # every B: one entry, one list read, settled; the hub (first size class only): a list per entry, settled with at most RA_SHORTCUT_LISTS of them
        sc = (c + (min(c, RA_SHORTCUT_LISTS + 1) if c <= RA_FIRST else 0), c + (1 if c <= RA_SHORTCUT_LISTS else 0))
        return Gadget(hubs + bs, n, [c] + [1] * c, removed=0, shortcut=sc)
    return Gadget(hubs + bs, n, [c + 1, c + 1] + [2] * c, removed=2 * c)


def blind_fan(rng, k, L, c, stem=False):
    """one-sided fan of c >= LONG_BUCKET reads behind a root and its neighbours (see the module text)"""
    assert c >= LONG_BUCKET
    rho, s = k + 20, 8
    m = -(-c // 90)
    assert L - 2 * rho >= 16 and m < LONG_BUCKET
    groups = [c // m + (1 if j < c % m else 0) for j in range(m)]
    while True:
        S = rnd(rng, L + s)
        R = S[L + s - rho:]
        hubs = [S[s:]] + ([S[:L]] if stem else [])
        U = "A" * 14 + rnd(rng, rho - 14)
        root = U + rnd(rng, L - rho)
        gs, bs = [], []
        for g in groups:
            T = rnd(rng, rho)
            gs.append(T + rnd(rng, L - 2 * rho) + U)
            bs += [R + rnd(rng, L - 2 * rho) + T for _ in range(g)]
        others = hubs + gs + bs
        if canonical(root) == root and all(canonical(x) > root for x in others):      # (the root is where the serial search of this gadget starts)
            break
    nh = len(hubs)
    lists = [c + nh - 1] * nh + [m] + [g + 1 for g in groups] + [nh + 1] * c
    pot = [c + 2 * (nh - 1)] * nh                                                     # own hits + twins, before the two entries of a pair seen from both sides merge
    return Gadget([root] + others, 1 + m + nh + c, lists, removed=2 * c if stem else 0, potential=pot, hidden=True)


def isolated(rng, L, n):
    return Gadget([rnd(rng, L) for _ in range(n)], n, [], shortcut=(0, 0))


def chain(rng, k, L, n, stride=10):
    """n reads tiling one random sequence: the ends are unresolved with one entry each (the candidate of their resolved neighbour), which nothing removes"""
    assert L - stride >= k + 10 and n >= 4
    S = rnd(rng, L + stride * (n - 1))
    return Gadget([S[i * stride:i * stride + L] for i in range(n)], 2, [1, 1], shortcut=(2, 2))


def flip_type(t):
    return 3 if t == 0 else 0 if t == 3 else t


def tandem(rng, k, L):
    """family E, two entries to one node: four reads over a tandem repeat (a unit of 7 bases, 12 times, between random flanks).  Two reads that both end or begin inside
    the repeat overlap at every shift that differs by a period, so a list names the same read several times (dupNode): the short cut leaves such a list to the walk.
    Built by search: what the lists are is the restatement's and the oracle's word (Model with a walk)."""
    assert L == 100 and k <= 40
    S = rnd(rng, 40) + rnd(rng, 7) * 12 + rnd(rng, 40)
    return Gadget([S[o:o + L] for o in (10, 20, 45, 60)])


def circle(rng, k, L):
    """family E, an earlier marker: three reads at 0, 40 and 80 of a circular sequence of 150 bases, and beside each a variant whose last 10 bases differ (so that no
    read has two unambiguous extensions).  A read's left neighbour a (overhang 70) comes first in its order, its right neighbour b (overhang 40) second, and b lies
    beyond a's far end: a's list continues r -> a to b.  The marker a of b is EARLIER in the order, so whether a is still in play at its turn matters (the sequential rule
    of :648): the short cut gives up and the walk marks the list.  Built by search, as `tandem`."""
    assert L == 100 and k <= 30
    C = rnd(rng, 150) * 2
    return Gadget([C[o:o + L] for o in (0, 40, 80)] + [C[o:o + L - 10] + rnd(rng, 10) for o in (0, 40, 80)])


def scatter(rng, k, L, seed):
    """family E, an earlier marker AND a nearer one: in `circle` the only marker of the node is the earlier one, so the short cut would also give up for want of a
    witness.  Here: reads at random places of a short circular sequence (some with an inverted part, so the strands mix) and variants with 12 other bases at an end --
    lists of 4 to 15 entries in which a node has markers on both sides of it.  The seeds were found by search with the restatement (Walk.shortcut_of with and without the
    rule): for some read the test for an earlier marker is the ONLY reason the short cut gives up.  The gadget draws from its own generator, so a seed names a read set."""
    assert L == 100 and k == 21
    rng = np.random.default_rng(seed)
    clen = int(rng.integers(120, 260)); C = rnd(rng, clen)
    if rng.random() < 0.5:
        a = int(rng.integers(0, clen - 60)); C = C[:a] + revcomp(C[a:a + 50]) + C[a + 50:]
    CC = C * 4
    n = int(rng.integers(4, 14)); offs = sorted(set(int(x) for x in rng.integers(0, clen, n)))
    reads = [CC[o:o + L] for o in offs]
    for o in offs:
        u = rng.random()
        if u < 0.35: reads.append(CC[o:o + L - 12] + rnd(rng, 12))
        elif u < 0.7: reads.append(rnd(rng, 12) + CC[o + 12:o + L])
    return Gadget(list(dict.fromkeys(reads)))


class Walk:
    """The reduce phase restated on strings, for the model: the hash table with its hidden buckets (hashTable.cpp:133-188, :111-123), the hits of a read
    (economyGraph.cpp:591-633), the serial search with its marks (:495-574, :643-679), and on the lists it leaves the marks' short cut of kernels_reduce.inc (ra_shortcut).
    Which reads are unresolved, and the two extension records of the resolved ones (their edges, :455-480), are the oracle's (Oracle.export_initial after the run).
    An entry is (to, type, len); ids are the oracle's (1-based rank of the canonical read).  Reads of one length only."""
    def __init__(self, reads, k, status, right, left):
        self.k, self.h = k, min(k, 64)
        canon = sorted(set(canonical(r) for r in reads))
        self.N = len(canon); assert self.N == len(status) - 1
        self.F = [None] + canon; self.R = [None] + [revcomp(r) for r in canon]
        self.L = len(canon[0]); assert all(len(r) == self.L for r in canon)
        self.unres = [False] + [int(status[i]) in (0, 1, 2) for i in range(1, self.N + 1)]      # (after the run: 1 explored, 2 marked; 4 resolved, 5 too many connections, 6 contained)
        h, L, table = self.h, self.L, {}
        for i in range(1, self.N + 1):
            for t, key in enumerate((self.F[i][:h], self.F[i][L - h:], self.R[i][:h], self.R[i][L - h:])):
                b = table.setdefault(key, [])
                if len(b) <= LONG_BUCKET:
                    b.append((i, t))
        self.table = {key: b for key, b in table.items() if len(b) < LONG_BUCKET}
        self.hidden = len(table) - len(self.table)
        self.adj = [[] for _ in range(self.N + 1)]
        for i in range(1, self.N + 1):                                     # the resolved reads' edges, in id order (:455-480)
            if int(status[i]) != 4:
                continue
            for rec, types in ((int(left[i]), (0, 1)), (int(right[i]), (3, 2))):
                to, o, ln = rec & ((1 << 40) - 1), (rec >> 40) & 3, rec >> 42
                if not (int(status[to]) == 4 and to < i):
                    self._insert(i, to, ln, types[0] if o == 0 else types[1])
        self.hitlist = [self.hits(i) if self.unres[i] else [] for i in range(self.N + 1)]
        self._search()
        self._potential()

    def _insert(self, u, v, delta, t):
        if u != v:
            self.adj[u].append((v, t, delta & 0xFFFFF)); self.adj[v].append((u, flip_type(t), (self.L - (self.L - delta)) & 0xFFFFF))

    def hits(self, r1):
        """verified overlaps of read r1 with other reads, as (to, type, len): what the explored filter (:605) then thins out"""
        h, k, L, out = self.h, self.k, self.L, []
        f1, c1 = self.F[r1], self.R[r1]
        for j in range(L - h + 1):
            for r2, t in self.table.get(f1[j:j + h], ()):
                if r2 == r1:
                    continue
                if t in (0, 2) and j <= L - k:
                    two = self.F[r2] if t == 0 else self.R[r2]
                    if f1[j + h:] == two[h:L - j]:
                        out.append((r2, 3 if t == 0 else 2, j))
                elif t in (1, 3) and j >= k - h:
                    two = self.R[r2] if t == 1 else self.F[r2]
                    s = L - j - h
                    if c1[s + h:] == two[h:L - s]:
                        out.append((r2, 0 if t == 1 else 1, L - j - h))
        return out

    def _explore(self, r1):
        if self.state[r1] != 0:
            return
        self.state[r1] = 1
        for r2, t, ln in self.hitlist[r1]:
            if self.state[r2] == 0:
                self._insert(r1, r2, ln, t)
        self.adj[r1].sort(key=lambda e: (e[2], e[0], e[1]), reverse=True)      # (:853-871)

    def _mark(self, r):
        self.length[r] = len(self.adj[r])
        mk = {e[0]: 1 for e in self.adj[r]}
        for a, t1, _ in self.adj[r]:
            if mk[a] != 1:
                continue
            for b, t2, _ in self.adj[a]:
                if mk.get(b) == 1 and ((t1 in (0, 2) and t2 in (0, 1)) or (t1 in (1, 3) and t2 in (2, 3))):
                    mk[b] = 2
        self.marked[r] = sum(mk[e[0]] == 2 for e in self.adj[r])
        self.state[r] = 2

    def _search(self):
        """:495-574 without the removals: a list is read by its neighbours' marks only before its own removals (kernels_reduce.inc, the head of the file), so the
        unreduced lists give the same marks -- tests/test_redgen_host.py holds the marked entries against the oracle's"""
        N = self.N
        self.state = [0] + [0 if self.unres[i] else 4 for i in range(1, N + 1)]
        self.length, self.marked = [0] * (N + 1), [0] * (N + 1)
        for i in range(1, N + 1):
            if self.state[i] != 0:
                continue
            queue, at = [i], 0
            while at < len(queue):
                r1 = queue[at]; at += 1
                self._explore(r1)
                if not self.adj[r1]:
                    continue
                if self.state[r1] == 1:
                    for r2, _, _ in list(self.adj[r1]):
                        if self.state[r2] == 0:
                            queue.append(r2); self._explore(r2)
                    self._mark(r1)
                if self.state[r1] == 2:
                    for r2, _, _ in list(self.adj[r1]):
                        if self.state[r2] != 1:
                            continue
                        for r3, _, _ in list(self.adj[r2]):
                            if self.state[r3] == 0:
                                queue.append(r3); self._explore(r3)
                        self._mark(r2)

    def _potential(self):
        """entries of the potential lists as k_rr_degp counts them: own hits on unresolved reads + hits of unresolved reads that point at the read"""
        self.potential = [0] * (self.N + 1)
        for i in range(1, self.N + 1):
            for r2, _, _ in self.hitlist[i]:
                if self.unres[r2]:
                    self.potential[i] += 1; self.potential[r2] += 1

    def shortcut_of(self, r, early_rule=True):
        """ra_shortcut on the final list of r: (lists read, settled, why not).  Lists of the first size class only; the others never try.
        early_rule=False: what it would do without its test for an earlier marker (tests/test_redgen_host.py: the case where that test alone decides)."""
        lst = sorted(self.adj[r], key=lambda e: (e[2], e[0], e[1]), reverse=True); n = len(lst)
        if n == 0 or n > RA_FIRST:
            return 0, False, "size"
        if len({e[0] for e in lst}) < n:
            return 0, False, "dup"
        order = {e[0]: x for x, e in enumerate(lst)}
        mk = {e[0]: 1 for e in lst}

        def one(x):
            a, t1, _ = lst[x]
            pm, early, wm = False, False, 0
            for b, t2, _ in self.adj[a]:
                if b in order and (lst[order[b]][1] & 1) == (flip_type(t2) >> 1):      # the twin b -> a continues r -> b: b is a potential marker of a
                    pm = True; early |= order[b] < x; wm = max(wm, order[b])
            if early and early_rule:
                return "early", pm, wm
            contra = False
            for b, t2, _ in self.adj[a]:
                if b in order and ((t1 ^ (t2 >> 1)) & 1) == 0:
                    if mk[b] == 3: contra = True
                    else: mk[b] = 2
            return ("contra" if contra else None), pm, wm
        lists = 0
        while True:
            unknown = [x for x in range(n) if mk[lst[x][0]] == 1]
            if not unknown:
                return lists, True, None
            x = unknown[-1]; sx = lst[x][0]
            lists += 1
            if lists > RA_SHORTCUT_LISTS:
                return lists, False, "limit"
            why, pm, w = one(x)
            if why:
                return lists, False, why
            if not pm:
                if mk[sx] == 1: mk[sx] = 3
                if mk[sx] != 3:
                    return lists, False, "self"
                continue
            if mk[sx] == 2:
                continue
            if w <= x or mk[lst[w][0]] != 2:
                return lists, False, "witness"
            lists += 1
            if lists > RA_SHORTCUT_LISTS:
                return lists, False, "limit"
            why, _, _ = one(w)
            if why or mk[sx] != 2:
                return lists, False, why or "witness"

    def shortcut(self):
        """(lists read, reads settled) over all unresolved reads, and how often the short cut declined for which reason"""
        lists = reads = 0; why = {}
        for r in range(1, self.N + 1):
            if self.unres[r]:
                a, ok, w = self.shortcut_of(r)
                lists += a; reads += ok
                if w: why[w] = why.get(w, 0) + 1
        return lists, reads, why


class Model:
    """what Context.reduce_stats() must report.  From the construction alone (`gadgets`), or -- with `walk`, the restatement over the oracle's records -- from the lists the
    serial search leaves, which adds the short cut's counters where the construction does not give them and serves the cases built by search (family E)."""
    def __init__(self, gadgets, walk=None):
        self.gadgets, self.walk = gadgets, walk
        built = not any(g.unresolved is None for g in gadgets)
        self.built = built
        if built:
            self.unresolved = sum(g.unresolved for g in gadgets)
            self.lists = sorted(x for g in gadgets for x in g.lists)
            self.potential = sorted(x for g in gadgets for x in g.potential)
            self.ranked = any(g.hidden for g in gadgets)
            self.removed = sum(g.removed for g in gadgets)
        self.shortcut = None if any(g.shortcut is None for g in gadgets) else tuple(sum(g.shortcut[x] for g in gadgets) for x in (0, 1))
        self.declined = None
        if walk is not None:
            un = [r for r in range(1, walk.N + 1) if walk.unres[r]]
            w = dict(unresolved=len(un), lists=sorted(walk.length[r] for r in un if walk.length[r]), ranked=walk.hidden > 0, removed=sum(walk.marked),
                     potential=sorted(walk.potential[r] for r in un if walk.potential[r] > RA_FIRST))
            if built:                                                      # (the construction and the restatement must agree)
                assert (self.unresolved, self.lists, self.ranked, self.removed) == (w["unresolved"], w["lists"], w["ranked"], w["removed"])
                assert all(x in w["potential"] for x in self.potential) and sum(x > RR_CAP for x in self.potential) == sum(x > RR_CAP for x in w["potential"])      # (the blind hubs' lists; a pair seen from both sides counts twice in the others')
            self.unresolved, self.lists, self.ranked, self.removed, self.potential = w["unresolved"], w["lists"], w["ranked"], w["removed"], w["potential"]
            a, b, self.declined = walk.shortcut()
            assert self.shortcut is None or self.shortcut == (a, b)
            self.shortcut = (a, b)

    def longest(self):
        return self.lists[-1] if self.lists else 0

    def stats(self, path):
        """Context.reduce_stats() on a reduce path of tests/test_gpu_parity.py (default, device, device_walk, host); None: not fixed by the model"""
        assert self.unresolved < DEVICE_REDUCE_MIN
        z = dict(form=0, unresolved=self.unresolved, lists_over_128=0, lists_over_512=0, shortcut_lists=0, shortcut_reads=0, removed=self.removed, potential_over_1024=0, slices=0)
        if self.unresolved == 0:
            return z
        if path in ("default", "host"):                    # (fewer unresolved reads than the library takes a device form for: the replay either way)
            z["form"] = 3
            return z
        z["form"] = 2 if self.ranked else 1
        z["lists_over_128"] = sum(x > RA_FIRST for x in self.lists)
        z["lists_over_512"] = sum(x > RA_CAP for x in self.lists)
        z["potential_over_1024"] = sum(x > RR_CAP for x in self.potential) if self.ranked else 0
        z["slices"] = 1 if self.ranked else 0
        if path == "device":
            z["shortcut_lists"], z["shortcut_reads"] = self.shortcut if self.shortcut is not None else (None, None)
        return z


class Case:
    def __init__(self, seed, k=21, L=100):
        self.seed, self.k, self.L, self.rng, self.gadgets = seed, k, L, np.random.default_rng(seed), []

    def add(self, maker, *a, **kw):
        self.gadgets.append(maker(self.rng, *a, **kw))
        return self

    def fan(self, c, stem=False):
        return self.add(fan, self.k, self.L, c, stem=stem)

    def blind(self, c, stem=False):
        return self.add(blind_fan, self.k, self.L, c, stem=stem)

    def filler(self, n_isolated=20, n_chain=30):
        self.add(isolated, self.L, n_isolated)
        return self.add(chain, self.k, self.L, n_chain)

    def reads(self):
        return [r for g in self.gadgets for r in g.reads]

    def arrays(self):
        """(bases, offsets) for reads_add_ascii, in an order shuffled by the seed (the input order must not matter)"""
        reads = self.reads()
        reads = [reads[x] for x in np.random.default_rng(self.seed + 1).permutation(len(reads))]
        bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
        off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
        return bases, off

    def walk(self, oracle):
        """the restatement over a finished oracle of this case's reads"""
        right, left, status, _ = oracle.export_initial()
        return Walk(self.reads(), self.k, status, right, left)

    def model(self, oracle=None):
        """the model from the construction alone, or with a finished oracle from the restatement too (Model)"""
        return Model(self.gadgets, self.walk(oracle) if oracle is not None else None)


def _len(n, seed, **kw):
    """family A: the longest list has exactly n entries and the marks remove some: a fan with a stem (n - 1 reads behind two hubs), blind beyond CONN_LIMIT"""
    def make():
        c = Case(seed, **kw)
        (c.blind if n - 1 >= 256 else c.fan)(n - 1, stem=True)
        return c.filler()
    return make


def _star(n, seed, filler=True, **kw):
    """pure fan of n reads: every entry of the hub's list at one overlap length (n <= 99), no removals, the short cut's counters known"""
    def make():
        c = Case(seed, **kw).fan(n)
        return c.filler() if filler else c
    return make


def _unresolved(n, seed):
    """exactly n unresolved reads: a fan of 3 and isolated reads"""
    return lambda: Case(seed).fan(3).add(isolated, 100, n - 4)


def _pot(n, seed):
    return lambda: Case(seed).blind(n).filler()


def case_empty(seed=431):
    """a blind fan WITHOUT the root: the search starts at the gadget's lowest id.  The hub: it sees nothing and every list stays empty.  A B: it explores H at once, H's
    list has that one entry and the other B keep empty lists."""
    c = Case(seed)
    g = blind_fan(c.rng, c.k, c.L, 120)
    m = len(g.reads) - 122                                                  # the root's neighbours; the root and they are left out
    hub, bs = g.reads[1], g.reads[2 + m:]
    one = canonical(hub) > min(canonical(b) for b in bs)
    c.gadgets.append(Gadget([hub] + bs, 121, [1, 1] if one else [], removed=0, shortcut=(2, 2) if one else (0, 0), hidden=True))
    return c.filler()


def case_dup(seed=456):
    c = Case(seed)
    return c.add(tandem, c.k, c.L).filler()


def case_early(seed=457):
    c = Case(seed)
    return c.add(circle, c.k, c.L).add(scatter, c.k, c.L, 5).add(scatter, c.k, c.L, 9).add(scatter, c.k, c.L, 57).filler()


def case_mixed(seed=440):
    """family H: one representative of every family in one read set (ranked form: a bucket is hidden)"""
    c = Case(seed)
    c.fan(9).fan(24).fan(25).fan(64, stem=True).fan(65).fan(128, stem=True).fan(255, stem=True)
    c.blind(512, stem=True).blind(1025).add(tandem, c.k, c.L).add(circle, c.k, c.L).add(scatter, c.k, c.L, 19)
    return c.filler(n_isolated=40, n_chain=60)


CASES = {"len64": _len(64, 401), "len65": _len(65, 402), "len128": _len(128, 403), "len129": _len(129, 404), "len256": _len(256, 405), "len257": _len(257, 406),
         "len512": _len(512, 407), "len513": _len(513, 408), "len1024": _len(1024, 409), "len1025": _len(1025, 410),
         "ties64": _star(64, 411), "ties65": _star(65, 412),
         "empty": case_empty, "single": _star(1, 421), "few1": _star(0, 422, filler=False), "few2": _star(1, 423, filler=False), "few3": _star(2, 424, filler=False),
         "few4": _star(3, 425, filler=False), "few5": _star(4, 426, filler=False), "unresolved1024": _unresolved(1024, 427), "unresolved1025": _unresolved(1025, 428),
         "sc_pre7": _star(7, 451), "sc_pre8": _star(8, 452), "sc_pre9": _star(9, 453), "sc_24": _star(24, 454), "sc_25": _star(25, 455), "sc_dup": case_dup, "sc_early": case_early,
         "nb129": _star(129, 461), "nb513": _pot(513, 462),
         "pot1024": _pot(1024, 471), "pot1025": _pot(1025, 472),
         "len129_k40": _len(129, 481, k=40, L=150), "len65_k55": _len(65, 482, k=55, L=250), "pot1025_k40": lambda: Case(483, k=40, L=150).blind(1025).filler(),
         "mixed": case_mixed}
# the property a case is named after, as tests/test_redgen_host.py proves it: longest list at mark time / unresolved reads / longest potential list
LONGEST = {"len64": 64, "len65": 65, "len128": 128, "len129": 129, "len256": 256, "len257": 257, "len512": 512, "len513": 513, "len1024": 1024, "len1025": 1025,
           "ties64": 64, "ties65": 65, "sc_pre7": 7, "sc_pre8": 8, "sc_pre9": 9, "sc_24": 24, "sc_25": 25, "nb129": 129, "nb513": 513, "pot1024": 1024, "pot1025": 1025,
           "len129_k40": 129, "len65_k55": 65, "pot1025_k40": 1025, "mixed": 1025}
UNRESOLVED = {"few1": 1, "few2": 2, "few3": 3, "few4": 4, "few5": 5, "unresolved1024": 1024, "unresolved1025": 1025}
POTENTIAL = {"pot1024": 1024, "pot1025": 1025, "pot1025_k40": 1025, "nb513": 513}


def get_case(name):
    return CASES[name]()
