"""Reads built to sit on the limits of run mode (kernels_probe_fast.inc), and a model of the route the kernel takes through them.  Plain numpy / Python.

The generator.  The locality order is (hash of the read's smallest hashed canonical 16-mer, strand | 255 - offset, id) -- k_minimizer_t, build_locality_order -- and the
hash is a multiplication by an odd constant mod 2^32, i.e. a bijection: the 16-mer whose hash is h is h * inverse(0x9E3779B1).  A LOCUS is a random stretch of genome with
that 16-mer (h = 1, 2, 3, 5, 6: each its own canonical form) planted into it; every read that covers it has it as its minimiser, so the reads of the locus stand at the
very front of the order, in an order the test decides: first the reads stored as the reverse complement of the genome (minimiser strand 0), latest genome start first,
then the reads stored as the genome (strand 1), earliest start first; the shift between neighbours is the difference of their starts.  Which way a read is stored is the
library's choice (the smaller of the read and its reverse complement); the locus decides it by the alphabet of two bases: a read that starts and ends in {A, C} is
smaller than its reverse complement (which starts with G or T), one that starts and ends in {G, T} is larger.

The model.  Context of a test: SAGE2OV_PROBE_TAIL=0, i.e. ONE launch of the sequential-groups clean form over all positions (plan_probe, launch_form), visits of
2^(chunkShift - 2) = 32 positions (FAST_CHUNK = 128 positions per block visit, FAST_WPB = 4 waves per block: k_probe_fast<S, NW, 2, 4, 0, 0, true, 2, true>), one visit per
wave.  `Model.route()` walks every visit as the kernel's read loop does -- the general path's start of a run, the plan of a step, the own-entry checks, step(), mirror(),
the moved ring -- on the reads' strings and a dictionary of the hash table's buckets, and returns the four run counters (Context.probe_run_stats) and a trace of the steps.
What it leaves out: a look-up by tag that returns another key's bucket (kernels_probe_fast.inc: 13 reads in 42.5 M), and reads the general path hands on for other reasons
than more than 128 candidates or an inconsistent candidate (none in a clean locus)."""
import numpy as np

MUL = 0x9E3779B1
INV = pow(MUL, -1, 1 << 32)
RUN_OFF, RUN_F, RUN_DMAX, RUN_NMAX, RUN_MMAX, RUN_LANES_MIN, CAP = 160, 1024, 64, 64, 16, 3, 128
VISIT = 32                       # positions of a nominal visit: 2^(chunkShift - log2(waves per block)) = 2^(7 - 2)
LONG_BUCKET = 100                # entries from which a bucket is a long one and never matches (hashTable.cpp:111-123)
_COMP = str.maketrans("ACGT", "TGCA")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canonical(s):
    r = revcomp(s)
    return s if s <= r else r


def mer_of_hash(h):
    """the 16-mer whose hash is h: two bits per base, A C G T = 0 .. 3, first base in the top bits"""
    v = (h * INV) & 0xFFFFFFFF
    return "".join("ACGT"[(v >> (30 - 2 * q)) & 3] for q in range(16))


def mer_value(m):
    v = 0
    for c in m:
        v = (v << 2) | _CODE[c]
    return v


def planted(h):
    """the 16-mer of hash h, which must be its own canonical form (not greater than its reverse complement)"""
    m = mer_of_hash(h)
    assert mer_value(m) <= mer_value(revcomp(m)), h
    return m


# ---------------------------------------------------------------------------------------------------------------- the minimiser, twice
def minimiser(read):
    """k_minimizer_t in numpy: (hash, meta) with meta = (255 - offset) | strand << 8; the smallest hash, first position wins"""
    a = np.frombuffer(read.encode(), dtype=np.uint8)
    code = ((a >> 1) & 3) ^ ((a >> 2) & 1)                  # A C G T -> 0 1 2 3 (ASCII 65 67 71 84)
    code = np.where(a == ord("G"), 2, np.where(a == ord("T"), 3, code)).astype(np.uint64)
    n = len(read) - 15
    if n <= 0:
        return 0xFFFFFFFF, 0
    f = np.zeros(n, dtype=np.uint64); r = np.zeros(n, dtype=np.uint64)
    for q in range(16):
        f = (f << np.uint64(2)) | code[q:q + n]
        r = r | ((np.uint64(3) - code[q:q + n]) << np.uint64(2 * q))
    hsh = (np.minimum(f, r) * np.uint64(MUL)) & np.uint64(0xFFFFFFFF)
    p = int(np.argmin(hsh))                                  # (the first of equal values)
    fw = int((int(f[p]) * MUL) & 0xFFFFFFFF) == int(hsh[p])
    return int(hsh[p]), (255 - min(p, 255)) | (256 if fw else 0)


def minimiser_naive(read):
    """the same, one position at a time over strings"""
    best, meta = 0xFFFFFFFF, 0
    for p in range(len(read) - 15):
        m = read[p:p + 16]; rc = revcomp(m)
        fv, rv = mer_value(m), mer_value(rc)
        hsh = (min(fv, rv) * MUL) & 0xFFFFFFFF
        if hsh < best:
            best, meta = hsh, (255 - min(p, 255)) | (256 if fv <= rv else 0)
    return best, meta


# ---------------------------------------------------------------------------------------------------------------- the generator
def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=n))


class Locus:
    """a random genome of `span` bases with the 16-mer of hash h at `mpos`, and reads of L bases at the genome starts `fw` (stored as the genome: minimiser strand 1) and
    `rc` (stored as its reverse complement: strand 0)."""

    def __init__(self, rng, h, L, fw=(), rc=(), mpos=None, span=None, free=(), period=None, palin=None):
        """free: genome starts of further reads that do not cover the planted 16-mer (they stand elsewhere in the order, by a minimiser of their own), bare or as
        (start, stored as the genome?); period = (x0, n, p):
        the genome repeats itself with period p over [x0, x0 + n + p); palin = (x0, n): the genome is its own reverse complement over [x0, x0 + n)"""
        fw, rc = sorted(fw), sorted(rc)
        free = [(f, None) if isinstance(f, int) else tuple(f) for f in free]; fdir = [f for f in free if f[1] is not None]; free = [f[0] for f in free]
        starts = fw + rc
        assert len(set(starts)) == len(starts), "one read per genome start (a read and its reverse complement are ONE read to the library)"
        self.h, self.L, self.M = h, L, planted(h)
        self.mpos = mpos if mpos is not None else (max(starts) if starts else 0) + 4
        span = span if span is not None else max(list(starts) + list(free) + [0]) + L + 4
        for s in starts:
            assert 0 <= s < self.mpos and s + L - 1 > self.mpos + 15 and s + L <= span, (s, self.mpos)
        for s in free:
            assert s + L <= span and (s > self.mpos or s + L < self.mpos + 16), "a free read covers the planted 16-mer"
        for attempt in range(400):
            g = list(rnd(rng, span))
            g[self.mpos:self.mpos + 16] = self.M
            if period:
                x0, n, p = period
                for x in range(x0 + n - 1, x0 - 1, -1): g[x] = g[x + p]
            if palin:
                x0, n = palin
                for q in range(n // 2): g[x0 + q] = g[x0 + n - 1 - q].translate(_COMP)
            want = {}
            for s, small in [(s, True) for s in fw] + [(s, False) for s in rc] + fdir:
                for q in (s, s + L - 1):
                    assert want.setdefault(q, small) == small, "a base that starts one read and ends another of the other strand"
            for q, small in want.items():
                g[q] = str(rng.choice(list("AC" if small else "GT")))
                if period:                                   # (the base's images under the period)
                    x0, n, p = period
                    for z in range(q % p, span, p):
                        if x0 <= min(z, q) and max(z, q) < x0 + n + p and z not in want: g[z] = g[q]
                if palin and palin[0] <= q < palin[0] + palin[1]:
                    z = 2 * palin[0] + palin[1] - 1 - q
                    assert z not in want; g[z] = g[q].translate(_COMP)
            self.genome = "".join(g)
            if self._good(fw, rc) and all(minimiser(canonical(self.genome[s:s + L]))[0] >= (1 << 16) for s in free) \
               and all((canonical(self.genome[s:s + L]) == self.genome[s:s + L]) == small for s, small in fdir):
                break
        else:
            raise AssertionError("no locus after 400 draws")
        self.fw, self.rc, self.free = fw, rc, sorted(free)

    def _good(self, fw, rc):
        g, L = self.genome, self.L
        for s in fw + rc:
            r = g[s:s + L]
            if (canonical(r) == r) != (s in fw) or r == revcomp(r):
                return False
            if minimiser_naive(r) != (self.h, (255 - (self.mpos - s)) | 256):          # no other 16-mer of the read hashes lower, none ties in front of it
                return False
        return True

    def read_at(self, s):
        return self.genome[s:s + self.L]

    def reads(self):
        """as the library stores them, in the order the locality order gives them: strand 0 by descending genome start, then strand 1 by ascending start"""
        return [revcomp(self.read_at(s)) for s in sorted(self.rc, reverse=True)] + [self.read_at(s) for s in self.fw]

    def free_reads(self):
        return [canonical(self.read_at(s)) for s in self.free]

    def expected_metas(self):
        L = self.L
        return [255 - ((s + L) - (self.mpos + 16)) for s in sorted(self.rc, reverse=True)] + [(255 - (self.mpos - s)) | 256 for s in self.fw]


def background(rng, n, L, taken=()):
    """n isolated random reads of L bases; no two share a minimiser hash with each other or with `taken`, none hashes below 2^16 (the planted ones stand in front)"""
    seen, out = set(taken), []
    while len(out) < n:
        r = rnd(rng, L)
        hsh, _ = minimiser(r)
        if hsh < (1 << 16) or hsh in seen:
            continue
        seen.add(hsh); out.append(r)
    return out


def to_arrays(reads, rng=None):
    """(bases, offsets) for reads_add_ascii, in a shuffled order when an rng is given (the input order must not matter)"""
    reads = list(reads)
    if rng is not None:
        reads = [reads[x] for x in rng.permutation(len(reads))]
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
    return bases, off


# ---------------------------------------------------------------------------------------------------------------- order, buckets, route
class Model:
    def __init__(self, reads, k):
        """reads: strings in any orientation and order; duplicates (either strand) are one read, as for the library"""
        self.k = k; self.h = min(k, 64)
        uniq = sorted(set(canonical(r) for r in reads))                      # id = 1 + rank of the canonical read (stringCompareInBytes: equal lengths -> lexicographic)
        self.N = len(uniq)
        mins = [minimiser(r) for r in uniq]
        order = sorted(range(self.N), key=lambda x: (mins[x][0], mins[x][1] & 0x1FF, x))      # LSD: 9 meta bits, then 32 hash bits, stable from id order
        self.idOf = [0] + [x + 1 for x in order]                                               # position (1-based) -> id
        self.seq = [""] + [uniq[x] for x in order]
        self.hash = [None] + [mins[x][0] for x in order]
        self.meta = [0xFFFF] + [mins[x][1] | (0x200 if p == 0 or mins[x][0] != mins[order[p - 1]][0] else 0) for p, x in enumerate(order)] + [0xFFFF]
        self.posOf = {self.idOf[p]: p for p in range(1, self.N + 1)}
        lens = set(len(r) for r in uniq)
        self.uniL = lens.pop() if len(lens) == 1 else 0
        self.maxL = max(len(r) for r in uniq)
        # the table: key (a k-mer as it stands, k <= 64: the whole window) -> entries position * 4 + type in bucket order = insertion order: ids ascending, then
        # type 0 prefix, 1 suffix, 2 prefix of the reverse complement, 3 suffix of the reverse complement (hashTable.cpp:94-109)
        self.bucket = {}
        h = self.h
        for x, r in enumerate(uniq):
            p = self.posOf[x + 1]; rc = revcomp(r)
            for t, key in enumerate((r[:h], r[len(r) - h:], rc[:h], rc[len(r) - h:])):
                self.bucket.setdefault(key, []).append(p * 4 + t)

    def entries(self, key):
        e = self.bucket.get(key, ())
        return () if len(e) >= LONG_BUCKET else e

    def long_buckets(self):
        return sum(1 for e in self.bucket.values() if len(e) >= LONG_BUCKET)

    def window_counts(self, p):
        s = self.seq[p]
        return [len(self.entries(s[j:j + self.h])) for j in range(len(s) - self.h + 1)]

    def tot(self, p):
        """slots of the read's ring: every entry of every window's bucket, its own included"""
        return sum(self.window_counts(p))

    def neighbours(self, p):
        """verified neighbours of a read all of whose candidates overlap it consistently (a clean locus): the slots that are not its own"""
        s = self.seq[p]
        return sum(1 for j in range(len(s) - self.h + 1) for e in self.entries(s[j:j + self.h]) if e >> 2 != p)

    def hits(self, p):
        """verified overlaps of read p as the reference counts them (economyGraph.cpp:79-438): every entry of every window's bucket but the read's own whose read equals
        this one over their whole overlap when laid where its type and the window put it (reads of one length: no containment)"""
        s = self.seq[p]; L = len(s); n = 0
        for j in range(L - self.h + 1):
            for e in self.entries(s[j:j + self.h]):
                r, t = e >> 2, e & 3
                if r == p: continue
                y = self.seq[r] if t < 2 else revcomp(self.seq[r]); st = j if t % 2 == 0 else j + self.h - len(y)
                lo, hi = max(st, 0), min(st + len(y), L)
                n += (st != 0 or len(y) != L) and s[lo:hi] == y[lo - st:hi - st]
        return n

    def capable(self):
        """runCapable(), and the instantiation with run mode exists (launch_fast_seq_any)"""
        L, k, h = self.uniL, self.k, self.h
        S = 4 if self.maxL <= 123 else (8 if self.maxL <= 251 else 16)       # words of a slot: the smallest power of two with 2 L + 9 <= 64 S
        NW = 8 if S == 4 else 10
        seq_form = L != 0 and self.maxL - h + 1 <= 128 and (S == 4 or (S == 8 and self.maxL <= 160))
        return bool(seq_form and h == k and L - k <= RUN_OFF and L <= 16 * NW and RUN_OFF + 2 * L - k <= RUN_F and L - h + 1 <= 128)

    def visits(self):
        """[first, end) positions of every visit: nominal ranges of VISIT positions whose start moves to the first read of the range with bit 9 (another minimiser hash)"""
        N = self.N; align = self.capable()
        def vb(g):
            s0 = g * VISIT
            if s0 >= N: return N
            if not align or g == 0: return s0
            for ln in range(VISIT):
                if s0 + ln < N and self.meta[1 + s0 + ln] & 0x200: return s0 + ln
            return s0
        return [(1 + vb(g), 1 + vb(g + 1)) for g in range((N + VISIT - 1) // VISIT)]

    # ---- the route
    def route(self, lanes_min=RUN_LANES_MIN, run_mode=True):
        """(reads off the ring, steps, of those reads by lanes, such steps), trace: one dict per step the run took or tried"""
        ctr = [0, 0, 0, 0]; trace = []
        if not (run_mode and self.capable()):
            return tuple(ctr), trace
        for first, end in self.visits():
            st = None; i = first
            while i < end:
                done = 0
                if st is not None:
                    done = self._continue(st, i, end, lanes_min, trace)
                    if done:
                        ctr[0] += done; ctr[1] += 1
                        if trace[-1]["lanes"]: ctr[2] += done; ctr[3] += 1
                        i += done; continue
                st = self._start(i)
                i += 1
        return tuple(ctr), trace

    def _start(self, i):
        """the general path took read i: the state of the run it starts, or None"""
        s = self.seq[i]; L = len(s); h = self.h; nwin = L - h + 1
        ring = []; wcnt = {}
        for j in range(nwin):
            e = self.entries(s[j:j + h]); wcnt[RUN_OFF + j] = len(e)
            ring += [(x, RUN_OFF + j) for x in e]
        if not 1 <= len(ring) <= CAP:
            return None
        F = [None] * (RUN_F + 64)
        F[RUN_OFF:RUN_OFF + L] = s
        gstart, glen = RUN_OFF, RUN_OFF + L
        for e, J in ring:
            r, t = e >> 2, e & 3
            if r == i:
                if not ((t == 0 and J == RUN_OFF) or (t == 1 and J == RUN_OFF + nwin - 1)): return None      # a palindromic own entry, or one in a foreign window
                continue
            y = self.seq[r] if t < 2 else revcomp(self.seq[r]); st = J if t % 2 == 0 else J + h - len(y)
            if st < 0 or st + len(y) > RUN_F: return None
            for q, c in enumerate(y):
                if F[st + q] is None: F[st + q] = c
                elif F[st + q] != c: return None                                                              # an inconsistent candidate: no run starts here
            gstart, glen = min(gstart, st), max(glen, st + len(y))
        if RUN_OFF - gstart > RUN_OFF: return None
        return dict(run=i, F=F, ring=ring, wcnt=wcnt, J0=RUN_OFF, gstart=gstart, glen=glen, off=self.meta[i] & 255, strand=(self.meta[i] >> 8) & 1, L=L)

    def _in_window(self, st, J, key):
        wc = st["wcnt"].get(J, 0)
        return wc <= 64 and any(e == key and j == J for e, j in st["ring"])

    def _step(self, st, dDrop, dr, info):
        """step(): 0 done, 1 the run ends, 2 no room (nothing touched)"""
        L, h = st["L"], self.h; nwin = L - h + 1; J0 = st["J0"]; F = st["F"]
        dropped = sum(1 for e, j in st["ring"] if j < J0 + dDrop)
        new = []
        for w in range(dr):
            Jw = J0 + nwin + w
            assert Jw + h <= st["glen"], "a key cut out of the frame behind its verified end"
            e = self.entries("".join(F[Jw:Jw + h])); new.append((Jw, e))
        nNew = sum(len(e) for _, e in new)
        info.update(nNew=nNew, tot_before=len(st["ring"]), dropped=dropped, max_window=max(len(e) for _, e in new))
        if nNew > RUN_NMAX or len(st["ring"]) - dropped + nNew > CAP:
            info.setdefault("refused", (len(st["ring"]) - dropped + nNew, nNew)); return 2
        fresh = []
        for Jw, e in new:
            st["wcnt"][Jw] = len(e); fresh += [(x, Jw) for x in e]
        good = True
        right = [(x, J) for x, J in fresh if x & 1 == 0]
        if right:
            eM, JM = right[-1]; reach = JM + L
            if reach > st["glen"]:
                if reach > RUN_F: good = False; info["frame_full"] = reach
                else:
                    y = self.seq[eM >> 2] if eM & 3 == 0 else revcomp(self.seq[eM >> 2])
                    for q in range(st["glen"], reach): F[q] = y[q - JM]
                    info["grown_by_type"] = eM & 3
                    st["glen"] = reach
        if good:
            for x, J in fresh:
                t = x & 3; y = self.seq[x >> 2] if t < 2 else revcomp(self.seq[x >> 2]); s0 = J if t % 2 == 0 else J + h - L
                inside = s0 >= st["gstart"] and s0 + L <= st["glen"]
                if not inside or list(y) != F[s0:s0 + L]:
                    good = False; info["failed_slot"] = (x, J, inside); break
        st["ring"] = [(e, j) for e, j in st["ring"] if j >= J0 + dDrop] + fresh
        st["base"] = st.get("base", 0) + dropped                                           # (the ring's start, not taken mod CAP)
        info["tot_after"] = len(st["ring"])
        return 0 if good else 1

    def _mirror(self, st):
        ring, h, L = st["ring"], self.h, st["L"]
        for a, b in zip(ring, ring[1:]):
            if a[1] == b[1] and a[0] >> 2 == b[0] >> 2: return False                       # a window holds one read twice
        by = {}
        for e, J in ring: by.setdefault(J, []).append(e)
        st["ring"] = [((e & ~3) | (3 - (e & 3)), RUN_F - (J + h)) for J in sorted(by, reverse=True) for e in by[J]]
        st["wcnt"] = {RUN_F - (J + h): c for J, c in st["wcnt"].items() if st["J0"] <= J < st["J0"] + L - h + 1}
        F = st["F"]
        st["F"] = [None if c is None else c.translate(_COMP) for c in reversed(F[:RUN_F])] + [None] * 64
        st["gstart"], st["glen"], st["J0"] = RUN_F - st["glen"], RUN_F - st["gstart"], RUN_F - (st["J0"] + L)
        st["base"] = 0
        return True

    def _continue(self, st, i, end, lanes_min, trace):
        """read i against the run: the number of reads answered (0: the run ends, the general path takes read i)"""
        L = st["L"]; meta = self.meta[i]; offR, strandR = meta & 255, (meta >> 8) & 1
        ok = meta != 0xFFFF
        flip = strandR != st["strand"]; d1 = offR - st["off"]; d2 = 0
        if flip:
            Mpos = st["J0"] + (255 - st["off"]); dl = Mpos + 16 + (255 - offR) - L - st["J0"]
            d1, d2 = max(dl, 0), max(-dl, 0); ok = ok and d1 <= RUN_DMAX and d2 <= RUN_DMAX
        else:
            ok = ok and 1 <= d1 <= RUN_DMAX
        info = dict(i=i, run=st["run"], flip=flip, d1=d1, d2=d2, m=1, lanes=False, ended=None, rc2=False, hash=self.hash[i]); trace.append(info)
        if not ok:
            info["ended"] = "shift"; return 0
        m = 1; rsx = [d1]; offs = [offR]
        if not flip:
            avail = min(RUN_MMAX - 1, end - i - 1); oP, DP = offR, d1
            for k2 in range(avail):
                mw = self.meta[i + 1 + k2]; o = mw & 255; dk = o - oP
                if mw == 0xFFFF or mw & 0x200 or (mw >> 8) & 1 != st["strand"] or dk < 1 or DP + dk > RUN_DMAX:
                    info["plan_cut"] = "none" if mw == 0xFFFF else ("bit9" if mw & 0x200 else ("strand" if (mw >> 8) & 1 != st["strand"] else ("dmax" if dk >= 1 else "offset"))); break
                oP = o; DP += dk; rsx.append(DP); offs.append(o); m += 1
            else:
                info["plan_cut"] = "mmax" if avail == RUN_MMAX - 1 else "visit"
            info["planned"] = m
            mm = 0
            while mm < m and self._in_window(st, st["J0"] + rsx[mm], (i + mm) << 2): mm += 1
            m = mm; ok = m >= 1
        elif d2 == 0:
            ok = self._in_window(st, st["J0"] + d1, (i << 2) | 2)
        if not ok:
            info["ended"] = "own entry"; return 0
        ph = 0
        while ph < 2 and ok:
            if ph == 1:
                if not flip: break
                ok = self._mirror(st)
                if not ok: info["ended"] = "mirror"; break
                if d2 > 0:
                    ok = self._in_window(st, st["J0"] + d2, i << 2)
                    if not ok: info["ended"] = "own entry"; break
                if d2 == 0: break
            dd = d1 if ph == 0 else d2; dn = (d1 if flip else rsx[m - 1]) if ph == 0 else d2
            if dn == 0: ph += 1; continue
            rc = self._step(st, dd, dn, info)
            if rc == 2 and not flip and m > 1:
                m = 1; info["rc2"] = True; continue
            ok = rc == 0
            if not ok: info["ended"] = "step %d" % rc
            if ok and flip: st["J0"] += dd
            ph += 1
        if not ok:
            return 0
        info["m"] = m
        if not flip:
            info["lanes"] = lanes_min != 0 and m >= lanes_min
            J0n = st["J0"] + rsx[m - 1]
            info["ring_at_records"] = len(st["ring"])
            info["ring_windows"] = sorted(set(j for _, j in st["ring"]))
            info["empty_edge_window"] = any(st["wcnt"].get(st["J0"] + rsx[r], 0) == 0 or st["wcnt"].get(st["J0"] + rsx[r] + L - self.h, 0) == 0 for r in range(m))
            info["ring_start"] = st.get("base", 0)
            nwin = L - self.h + 1
            info["ranges"] = [(sum(1 for _, j in st["ring"] if j < st["J0"] + rsx[r]), sum(1 for _, j in st["ring"] if j < st["J0"] + rsx[r] + nwin)) for r in range(m)]
            st["base"] = st.get("base", 0) + sum(1 for _, j in st["ring"] if j < J0n)
            st["ring"] = [(e, j) for e, j in st["ring"] if j >= J0n]
            st["J0"] = J0n; st["off"] = offs[m - 1]
            return m
        st["off"] = offR; st["strand"] = strandR
        return 1


# ---------------------------------------------------------------------------------------------------------------- the cases
HASHES = [1, 2, 3, 5, 6, 9, 18, 19, 21, 22, 25, 37, 38, 41, 53, 54, 55, 57, 58, 61, 65, 71, 73, 74, 77]      # own canonical form each, no two a shift of each other (h, 4 h)


class Case:
    """a read set: loci {name: Locus} in the order of their hashes (= of their positions: they stand in front of every background read), background reads, k"""

    def __init__(self, seed, k=40, L=150, n_background=1500):
        self.rng = np.random.default_rng(seed); self.k, self.L, self.nbg = k, L, n_background
        self.loci = {}; self.extra = []; self._model = None

    def locus(self, name, **kw):
        h = kw.pop("h", None) or HASHES[len(set(l.h for l in self.loci.values()))]
        self.loci[name] = Locus(self.rng, h, kw.pop("L", self.L), **kw)
        return self.loci[name]

    def reads(self):
        if not hasattr(self, "_reads"):
            own = [r for l in self.loci.values() for r in l.reads() + l.free_reads()] + list(self.extra)
            self._reads = own + background(self.rng, self.nbg, self.L, taken=[l.h for l in self.loci.values()])
        return self._reads

    def arrays(self):
        return to_arrays(self.reads(), np.random.default_rng(7))

    def model(self):
        if self._model is None: self._model = Model(self.reads(), self.k)
        return self._model

    def first_pos(self, name):
        """position of the locus's first read (the loci stand in the order of their hashes, a hash shared by two loci interleaves them: not for those)"""
        p = 1
        for l in sorted(set(x.h for x in self.loci.values())):
            if l == self.loci[name].h: return p
            p += sum(len(x.reads()) for x in self.loci.values() if x.h == l)
        raise KeyError(name)

    def positions(self, name):
        """positions of the locus's reads (those that cover the planted 16-mer), ascending"""
        m = self.model(); own = set(self.loci[name].reads())
        return [p for p in range(1, m.N + 1) if m.seq[p] in own]

    def steps_of(self, name, trace):
        l = self.loci[name]
        return [t for t in trace if t["hash"] == l.h]


def case_shifts(seed=301):
    """A: two reads 1, 63, 64, 65 bases apart, a chain of shifts of 64, one hash in two unrelated loci (offset difference 0 and 5 between reads of different genomes)"""
    c = Case(seed)
    for d in (1, 63, 64, 65):
        c.locus("d%d" % d, fw=[10, 10 + d], mpos=100)
    c.locus("chain64", fw=[5, 69, 133], mpos=135)
    x = c.locus("twoX", fw=[50, 60], mpos=100)                       # offsets 50, 40
    c.locus("twoY", h=x.h, fw=[70, 75], mpos=120)                    # offsets 50, 45: order by offset 50, 50 (by id), 45, 40
    return c


def case_mirror(seed=302):
    """B: strand changes.  A locus of one read stored as the reverse complement (at genome start sr) and reads stored as the genome (first at sf): the second strand's first
    read starts dl = sr - sf bases behind the current read in the frame's direction: dl > 0 a forward step d1 before the mirror, dl < 0 a step d2 after it."""
    c = Case(seed)
    for d in (1, 64, 65):
        c.locus("d1_%d" % d, rc=[20 + d], fw=[20, 23], mpos=100)
        c.locus("d2_%d" % d, rc=[20], fw=[20 + d, 23 + d], mpos=100)
    c.locus("both", rc=[30, 33, 40], fw=[28, 29, 31, 36], mpos=100)   # a run on strand 0, the mirror, a run on strand 1
    x = c.locus("dl0_X", rc=[20], mpos=100)                           # dl = 0 between reads of two unrelated genomes (within one genome the two would be ONE read):
    c.locus("dl0_Y", h=x.h, fw=[20, 23], mpos=100)                    # the mirror is asked for without a step, the own entry is not there
    return c


def case_plans(seed=303):
    """C: the plan of a step.  Chains at shift 1 of 16, 17, 18 and 34 reads (the first read of a locus takes the general path: steps of 15, 16, 16 + 1, 16 + 16 + 1 reads),
    shifts of 5 (12 reads reach 60, the 13th 65), loci of 3 and 4 reads (steps of RUN_LANES_MIN - 1 and RUN_LANES_MIN reads), a plan ended by the other strand"""
    c = Case(seed)
    c.locus("n3", fw=[10, 11, 12], mpos=100); c.locus("n4", fw=[10, 11, 12, 13], mpos=100)
    c.locus("strand", rc=[40, 41, 42, 43], fw=[37, 38, 39], mpos=100)
    c.locus("n16", fw=list(range(10, 26)), mpos=100)                  # positions 15 .. 30 (the first visit ends behind it)
    c.locus("n17", fw=list(range(10, 27)), mpos=100)
    c.locus("shift5", fw=list(range(5, 5 + 5 * 15, 5)), mpos=100)
    c.locus("n18", fw=list(range(10, 28)), mpos=100)
    c.locus("n34", fw=list(range(10, 44)), mpos=100)
    return c


def case_ring(seed=304, n=(126, 127, 128)):
    """D: blocks of n reads at consecutive starts, alternating strands in groups: a read in the middle of a block of n has every read of the block within 110 bases on
    either side: n + 1 slots (its own two among them) = CAP - 1, CAP, CAP + 1"""
    c = Case(seed, n_background=1200)
    for x in n:
        starts = list(range(140 - x, 140)); rc = [s for s in starts if (s // 8) % 3 == 1]; fw = [s for s in starts if s not in rc]
        c.locus("n%d" % x, fw=fw, rc=rc, mpos=141)
    return c


def case_dense_fw(seed=305):
    """D: blocks of 127 and 100 reads of ONE strand at consecutive starts: long runs whose ring fills up to CAP (steps that find no room and are retried with one read),
    whose start wraps past CAP, and whose slot ranges cross slot 64"""
    c = Case(seed, n_background=1200)
    c.locus("fw127", fw=list(range(13, 140)), mpos=141)
    c.locus("fw100", fw=list(range(40, 140)), mpos=141)
    return c


def case_wrap(seed=305):
    """D: a ring whose start goes round.  A run drops the slots of the windows it passes: the prefix entries of the reads that start there and the suffix entries of the
    reads that start 110 bases earlier.  4 starts in 7 over 240 bases on either side of the minimiser (reads that do not cover it included, left and right) keep a read's
    ring below CAP while the 19 reads of strand 1, 7 bases apart and all in one visit (the locus in front fills the visit before), drop more than CAP slots between them."""
    c = Case(seed, n_background=600); mp = 260
    fw = list(range(mp - 133, mp, 7))
    dens = [s for s in range(17, mp + 100) if s % 7 in (0, 1, 3, 5) and s not in fw]
    rc = [s for s in dens if mp - 133 <= s < mp]; free = [s for s in dens if s < mp - 134 or s > mp]
    c.locus("fill", fw=list(range(10, 10 + (-len(rc)) % VISIT)), mpos=141)
    c.locus("wrap", fw=fw, rc=rc, free=free, mpos=mp)
    return c


def case_visits(seed=306):
    """H: loci of 32, 31 and 32 reads: the minimiser changes at items 32 (the first position of the nominal visit range [32, 64)), 63 and 95 (the last position of
    [64, 96)); then groups of 63, 64, 65 reads and the largest the generator makes: a read of 150 bases holds the 16-mer at 135 offsets, the generator uses the 133 that
    leave the read's first and last base free (they decide which way the read is stored); a read and its reverse complement are one read to the library, so the second
    strand's 133 come from a second locus with the same hash"""
    c = Case(seed, n_background=1200)
    c.locus("a32", fw=list(range(10, 42)), mpos=100); c.locus("b31", fw=list(range(10, 41)), mpos=100); c.locus("c32", fw=list(range(10, 42)), mpos=100)
    for x in (63, 64, 65):
        c.locus("g%d" % x, fw=list(range(10, 10 + 2 * x, 2)), mpos=141)
    big = c.locus("big_fw", fw=list(range(8, 141)), mpos=141)
    c.locus("big_rc", h=big.h, rc=list(range(8, 141)), mpos=141)
    return c


def case_capability(k, L=150, seed=307, mixed=False):
    """G: one chain of 20 reads at shift 1 and one with a strand change, at the k and L of the capability edge; mixed: one background read a base shorter"""
    c = Case(seed + 13 * k + L, k=k, L=L, n_background=600)
    m = L - 40
    c.locus("chain", fw=list(range(m - 30, m - 10)), mpos=m)
    c.locus("mirror", rc=[m - 20, m - 18], fw=[m - 25, m - 24, m - 21], mpos=m)
    if mixed: c.extra.append(rnd(c.rng, L - 1))
    return c


CAPABILITY = {"k23_128_windows": (dict(k=23), True), "k22_129_windows": (dict(k=22), False), "k64": (dict(k=64), True), "k65": (dict(k=65), False),
              "mixed_lengths": (dict(k=40, mixed=True), False), "four_words_L100_k21": (dict(k=21, L=100), True), "eight_words_L160_k33": (dict(k=33, L=160), True)}


def mutated(read, q):
    """the read with base q replaced by the next base of the alphabet"""
    return read[:q] + "ACGT"[("ACGT".index(read[q]) + 1) % 4] + read[q + 1:]


def case_compares(seed=308, k=40, L=150):
    """E: the compares of a step's new slots.  new_n: a step of one read whose d new windows hold n slots -- the read's own suffix entry and those of n - 1 reads of the
    other strand that start between the two (CP = 64 / NW slots a pass, RUN_NPRE = 3 passes loaded up front: 3 CP slots take three passes, 3 CP + 1 the first pass beyond);
    grow0 / grow2: a new window with the prefix entry of a read stored as the genome / as its reverse complement, which reaches past the frame's end;
    mut_*: a read that shares the k-mer of a new window and differs from the genome in one base: in its first dword (found by its suffix entry), in its last dword and in its
    last base (found by its prefix entry; a genuine read one base further right brings the frame up to there in the same step)"""
    c = Case(seed + k + L, k=k, L=L, n_background=1000)
    cp = 64 // (8 if L <= 123 else 10); off = L - 17; a = 8
    for n in (3 * cp, 3 * cp + 1):
        c.locus("new_%d" % n, fw=[a, a + n + 2], rc=list(range(a + 1, a + n)), mpos=a + off)
    nw = L - k + 1
    c.locus("grow0", fw=[a, a + 9], mpos=a + 20, free=[(a + nw + 4, True)])
    c.locus("grow2", fw=[a, a + 9], mpos=a + 20, free=[(a + nw + 4, False)])
    l = c.locus("mut_first_dword", fw=[a, a + 2], mpos=a + 3)
    c.extra.append(canonical(mutated(l.read_at(a + 1), 3)))
    for name, q in (("mut_last_dword", L - 6), ("mut_last_base", L - 1), ("mut_middle", L // 2)):
        l = c.locus(name, fw=[a, a + 2], mpos=a + 20, free=[a + nw + 1], span=a + nw + L + 8)
        c.extra.append(canonical(mutated(l.read_at(a + nw), q)))
    return c


def case_limits(seed=309):
    """D / E / F: nmax_64 / nmax_65: a step of one read at shift 64 whose new windows hold 64 / 65 slots (RUN_NMAX); frame_full: one read of strand 0 with the minimiser at
    its start, reads of strand 1 up to the minimiser at their end, and a neighbour 100 bases further right: its reach lies behind RUN_F;
    win_64 / win_65: 63 / 64 unrelated reads that end in the k-mer a read of the run ends in: a new window of 64 / 65 entries"""
    c = Case(seed, n_background=1000); a = 8; m = a + 133
    c.locus("nmax_64", fw=[a, a + 64], rc=list(range(a + 1, a + 64)), mpos=m)
    c.locus("nmax_65", fw=[a, a + 64], rc=list(range(a + 1, a + 64)), mpos=m, free=[a + 140])
    c.locus("frame_full", rc=[a], fw=[a + 1, a + 60, a + 120, a + 132], mpos=m, free=[a + 232])
    for n in (64, 65):
        l = c.locus("win_%d" % n, fw=[a, a + 2], mpos=a + 20)
        x = l.read_at(a + 2)[-c.k:]
        c.extra += [rnd(c.rng, c.L - c.k) + x for _ in range(n - 1)]
    return c


def case_twice(seed=310):
    """B / F: a window that holds one read twice.
    palindrome: the genome is its own reverse complement over the 260 bases around the k-mer P at J (P is its own reverse complement, k even).  The read Q that starts at J
    has P as its prefix k-mer AND as the suffix k-mer of its reverse complement: the bucket of P holds (Q, 0) and (Q, 3), and both are true overlaps wherever P's window
    is in a ring -- Q lies on the frame from J on, its reverse complement up to J + k.  The reads of both strands a few bases in front of J have that window: at their
    strand change mirror() finds one read twice in a window and declines.  Q itself starts no run (a palindromic own entry), and neither does any read that starts inside
    the palindrome: its reverse complement lies on the genome too, within 110 bases of it, so its own type-2 entry sits in one of its windows.  The run is therefore
    started by the read of strand 0 at J + 1, whose reverse complement starts one base in front of the mirror image of the palindrome; the read at J - 2 continues it
    (window J enters the ring with that step), the read of strand 1 at J - 5 asks for the mirror.
    self_again: the genome repeats itself with period L - k over 260 bases: every read inside has its prefix k-mer again as its suffix k-mer, i.e. in its last window
    (own entries of both types in one window: no run starts there), and the copies of the k-mer at the ends of the repeat hold entries that are no overlaps."""
    c = Case(seed, n_background=1000); J = 130
    c.locus("palindrome", rc=[J + 1, J - 2], fw=[J - 5, J], mpos=J + 60, palin=(J - 110, 260), span=J + 160)
    c.locus("self_again", rc=[J - 6, J - 3], fw=[J - 5, J - 2, J], mpos=J + 60, period=(J - 110, 150, 110), span=J + 160)
    return c


def case_full_ring(seed=311):
    """D / F: a ring of exactly CAP slots inside a planned step, with an empty window last in a read's range, which only a LONG bucket gives (a read's first window holds
    its own prefix entry -- the own-entry check has just found it --, its last window its own suffix entry): 113 reads of one strand at consecutive starts, and 100
    unrelated reads that end in the k-mer the 17th of them ends in -- that bucket has 101 entries and matches nothing.  The step that ends on that read would hold 129 slots
    with the entry; without it the ring is full and the read's last window, the ring's last, reads as 'first slot 0, no slots' (ambB in records())."""
    c = Case(seed, n_background=800)
    l = c.locus("block", fw=list(range(27, 140)), mpos=141)
    x = l.read_at(43)[-c.k:]
    c.extra += [rnd(c.rng, c.L - c.k) + x for _ in range(100)]
    return c


CASES = {"shifts": case_shifts, "mirror": case_mirror, "plans": case_plans, "ring": case_ring, "dense": case_dense_fw, "wrap": case_wrap, "visits": case_visits,
         "full_ring": case_full_ring, "compares": case_compares, "compares_L100": lambda: case_compares(k=21, L=100), "limits": case_limits, "twice": case_twice}
for _n, (_kw, _cap) in CAPABILITY.items():
    CASES[_n] = (lambda kw=_kw: case_capability(**kw))
_built = {}


def get_case(name):
    """the case, built once per process"""
    if name not in _built: _built[name] = CASES[name]()
    return _built[name]
