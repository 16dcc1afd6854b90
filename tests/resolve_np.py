"""The numpy statement of whitelist abundance and the resolution of ambiguous barcodes (include/ibu_hip.h: ibu_abundance_add,
ibu_abundance_counts, ibu_resolve_barcodes), written from the header comment alone, on top of whitelist_np.classify.  Test
infrastructure: the product never imports it.

An abundance holds one counter per whitelist entry, all zero at first.  add: a record contributes when there are no class
bytes, or when its class c < 8 has bit c of class_mask set; the counter of low = barcode & mask(2*bc_len) grows by one where low
is in the whitelist.  resolve: for every record of class 2 the candidates are the neighbours of low that are in the whitelist,
total the sum of their counters and best the largest; best > 0 and best * den >= num * total moves the record onto that
candidate (the bits above 2*bc_len stay) and makes its class 4; everything else stays."""
import math

import numpy as np

from tests import whitelist_np as wnp

RESOLVED = 4
REC = wnp.REC
TOTALS = ("examined", "resolved", "below_share", "unseen")


class Abundance:
    """The counters of a whitelist: `wl` its distinct codes, ascending, `n[k]` the counter of wl[k]."""

    def __init__(self, whitelist, bc_len):
        self.wl = np.unique(np.asarray(whitelist, dtype=np.uint64))
        self.bc_len = bc_len
        self.n = np.zeros(len(self.wl), np.uint64)

    def reset(self):
        self.n[:] = 0

    def copy(self):
        c = Abundance(self.wl, self.bc_len)
        c.n = self.n.copy()
        return c


def _barcodes(recs_or_bc):
    a = np.asarray(recs_or_bc)
    return a["barcode"] if a.dtype.names else a.astype(np.uint64)


def _find(ab, keys):
    """-> (position of every key in ab.wl, whether it is there)."""
    pos = np.searchsorted(ab.wl, keys)
    pos[pos == len(ab.wl)] = 0
    return pos, ab.wl[pos] == keys


def legal_share(num, den):
    return 1 <= num <= den < 1 << 24 and 2 * num > den


def add(ab, recs, cls=None, class_mask=1, times=1):
    """ibu_abundance_add (`times` calls over the same records)."""
    bc = _barcodes(recs)
    on = np.ones(len(bc), bool) if cls is None else (np.asarray(cls) < 8) & (((class_mask >> np.minimum(np.asarray(cls), 7).astype(np.uint32)) & 1) == 1)
    low = bc[on] & wnp.mask(ab.bc_len) if ab.bc_len < 32 else bc[on]
    pos, hit = _find(ab, low)
    ab.n += np.bincount(pos[hit], minlength=len(ab.wl)).astype(np.uint64) * np.uint64(times)
    return ab


def counts(ab, codes):
    """ibu_abundance_counts."""
    codes = np.asarray(codes, dtype=np.uint64)
    pos, hit = _find(ab, codes)          # a code with bits at or above 2*bc_len is not in the whitelist: no entry has such bits
    return np.where(hit, ab.n[pos], np.uint64(0)).astype(np.uint64)


def resolve(ab, recs, cls, num, den):
    """ibu_resolve_barcodes -> (records, class bytes, {"examined", "resolved", "below_share", "unseen"})."""
    if not legal_share(num, den):
        raise ValueError("1 <= num <= den < 2^24 and 2 * num > den")
    recs = np.ascontiguousarray(recs).view(REC).reshape(-1).copy()
    cls = np.asarray(cls, dtype=np.uint8).copy()
    m = wnp.mask(ab.bc_len) if ab.bc_len < 32 else np.uint64(wnp.FREE)
    rows = np.flatnonzero(cls == wnp.AMBIGUOUS)
    low = recs["barcode"][rows] & m
    total = np.zeros(len(rows), np.uint64)
    best = np.zeros(len(rows), np.uint64)
    winner = np.zeros(len(rows), np.uint64)
    for i in range(ab.bc_len):
        for x in (1, 2, 3):
            nb = low ^ np.uint64(x << (2 * i))
            pos, hit = _find(ab, nb)
            c = np.where(hit, ab.n[pos], np.uint64(0))
            total += c
            better = hit & (c > best)
            winner = np.where(better, nb, winner)
            best = np.where(better, c, best)
    ok = (best > 0) & (best * np.uint64(den) >= np.uint64(num) * total)   # counters below 2^40, den < 2^24: no overflow
    recs["barcode"][rows[ok]] = (recs["barcode"][rows[ok]] & ~m) | winner[ok]
    cls[rows[ok]] = RESOLVED
    tot = {"examined": len(rows), "resolved": int(ok.sum()), "below_share": int((~ok & (total > 0)).sum()), "unseen": int((total == 0).sum())}
    return recs, cls, tot


# ---- brute force: Python dicts and a Hamming loop over the whitelist --------------------------------------------------------
def _one_apart(a, b):
    d = a ^ b
    pairs = (d | (d >> 1)) & 0x5555555555555555
    return pairs != 0 and pairs & (pairs - 1) == 0


def brute_add(table, whitelist, bc_len, barcodes, cls=None, class_mask=1):
    """`table`: dict code -> count (missing: 0), updated in place."""
    m = (1 << (2 * bc_len)) - 1
    wls = {int(c) for c in whitelist}
    for k, b in enumerate(int(v) for v in barcodes):
        if cls is not None and not (int(cls[k]) < 8 and (class_mask >> int(cls[k])) & 1):
            continue
        if b & m in wls:
            table[b & m] = table.get(b & m, 0) + 1
    return table


def brute_resolve(table, whitelist, bc_len, barcodes, cls, num, den):
    """-> (barcodes, classes, totals, the largest number of candidates of one record that pass the share test)."""
    m = (1 << (2 * bc_len)) - 1
    wl = sorted({int(c) for c in whitelist})
    out, oc = [int(v) for v in barcodes], [int(c) for c in cls]
    tot = dict.fromkeys(TOTALS, 0)
    most = 0
    for k, b in enumerate(out):
        if oc[k] != 2:
            continue
        tot["examined"] += 1
        cand = [c for c in wl if _one_apart(b & m, c)]
        total = sum(table.get(c, 0) for c in cand)
        passing = [c for c in cand if table.get(c, 0) > 0 and table.get(c, 0) * den >= num * total]
        most = max(most, len(passing))
        if passing:
            out[k] = (b & ~m) | passing[0]
            oc[k] = RESOLVED
            tot["resolved"] += 1
        elif total:
            tot["below_share"] += 1
        else:
            tot["unseen"] += 1
    return np.array(out, np.uint64), np.array(oc, np.uint8), tot, most


# ---- case builders, shared by tests/test_resolve_host.py and tests/test_gpu_resolve.py ---------------------------------------
def records(rng, bc):
    recs = np.zeros(len(bc), REC)
    recs["barcode"] = bc
    recs["umi"] = rng.integers(0, 1 << 63, len(bc), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(bc), dtype=np.uint64)
    recs["index"] = np.arange(len(bc), dtype=np.uint64)
    return recs


def make_case(rng, bc_len, w, n, junk=True):
    """-> (whitelist, barcodes[n]).  The whitelist of whitelist_np.make_case (its planted pair at distance 2 included) with up to 32
    more such pairs planted: entry 2 + k gets a partner two substitutions away, which takes the place of entry w - 1 - k.  The
    barcodes, shuffled: 60 % exact reads drawn with a skew towards the front of the whitelist (entry floor(live * u^3), u uniform:
    a pair's first entry has many reads and its partner few, so that pairs near the front resolve at 39/40 and pairs further back
    do not), none at all of the last quarter of the planted pairs (their midpoints are `unseen`); 20 % one substitution of a random
    entry; 10 % midpoints of the planted pairs; 10 % uniform random.  Junk bits above 2*bc_len on half of them below 32 bases."""
    wl, _ = wnp.make_case(rng, bc_len, w, 16, junk=False)
    wl = wl.copy()
    w = len(wl)
    pairs = [(int(wl[0]), int(wl[1]))] if w >= 2 and bc_len >= 2 else []
    extra = min(32, max(0, (w - 2) // 4)) if bc_len >= 2 else 0
    have = {int(c) for c in wl}
    for k in range(extra):
        a = int(wl[2 + k])
        i, j = (int(v) for v in rng.permutation(bc_len)[:2])
        b = a ^ (int(rng.integers(1, 4)) << (2 * i)) ^ (int(rng.integers(1, 4)) << (2 * j))
        if b in have:
            continue
        have.discard(int(wl[w - 1 - k]))
        wl[w - 1 - k] = b
        have.add(b)
        pairs.append((a, b))
    silent = pairs[len(pairs) - len(pairs) // 4:]
    mute = np.array([c for p in silent for c in p], np.uint64)
    live = wl[~np.isin(wl, mute)] if len(mute) else wl
    mids = []
    for a, b in pairs:                                   # the two barcodes between a and b: one of the two substitutions each
        d = a ^ b
        first = d & (3 << (2 * (((d & -d).bit_length() - 1) // 2)))   # the lowest base in which they differ
        mids += [a ^ first, b ^ first]
    shares = [int(round(s * n)) for s in (0.6, 0.2, 0.1, 0.1)]
    shares[0] += n - sum(shares)
    exact = live[np.minimum((len(live) * rng.random(shares[0]) ** 3).astype(np.int64), len(live) - 1)]
    sub = wnp.substitute(rng, wl[rng.integers(0, w, shares[1])], bc_len)
    mid = np.array(mids if mids else [int(wl[0])], np.uint64)[rng.integers(0, max(len(mids), 1), shares[2])]
    rnd = wnp.random_codes(rng, bc_len, shares[3])
    bc = rng.permutation(np.concatenate([exact, sub, mid, rnd]))
    return wl, (wnp.with_junk(rng, bc, bc_len) if junk else bc)


def chain(wl, bc_len, recs, num=39, den=40, class_mask=1):
    """correct -> add (the classes of class_mask) -> resolve, in numpy -> (records, classes, totals, abundance)."""
    want, cls, _ = wnp.correct_records(recs, wl, bc_len, 1)
    ab = add(Abundance(wl, bc_len), want, cls, class_mask)
    out, cls2, tot = resolve(ab, want, cls, num, den)
    return out, cls2, tot, ab


SHARES = [(1, 1), (3, 4), (39, 40), ((1 << 23) + 1, (1 << 24) - 1)]


def boundary_counts(num, den):
    """Counter tuples of the candidates of one midpoint each, around best * den == num * total, with what resolve must say and
    which candidate wins.  (nr, dr) = num / den in lowest terms: best = nr and total = dr is the smallest case of equality."""
    g = math.gcd(num, den)
    nr, dr = num // g, den // g
    rest = dr - nr
    a = rest // 2
    out = [((nr, rest), "resolved", 0),                       # equality
           ((rest, nr), "resolved", 1),                       # ... with the winner second
           ((nr - 1, rest), "below_share" if nr - 1 + rest else "unseen", None),   # one read fewer
           ((0, 0), "unseen", None),
           ((nr, a, rest - a), "resolved", 0),                # three candidates
           ((a, rest - a, nr), "resolved", 2),
           ((a, nr - 1, rest - a), "below_share" if nr - 1 + rest else "unseen", None),
           ((2 * nr, 2 * rest + 1), "below_share", None),     # past equality on the other side
           ((7, 0), "resolved", 0)]                           # a candidate without reads does not stand in the way
    return out


def boundary_case(bc_len, num, den, seed=0):
    """-> (whitelist, [(code, count)], midpoints, expected outcome per midpoint, expected low bits per midpoint).  One random
    midpoint per boundary_counts() entry; its candidates are its neighbours 1, 3 * (bc_len - 1) and 4 (three bases apart from each
    other pairwise: no candidate is a neighbour of another midpoint's)."""
    rng = np.random.default_rng([0x1B00700, bc_len, num, den, seed])
    specs = boundary_counts(num, den)
    centres = [int(c) for c in wnp.random_codes(rng, bc_len, len(specs))]
    wl, setc, outcome, low = [], [], [], []
    for c, (cnts, what, win) in zip(centres, specs):
        cand = [wnp.neighbour(c, j) for j in (1, 3 * (bc_len - 1), 4)[:len(cnts)]]
        wl += cand
        setc += list(zip(cand, cnts))
        outcome.append(what)
        low.append(cand[win] if win is not None else c)
    return np.array(wl, np.uint64), setc, np.array(centres, np.uint64), outcome, np.array(low, np.uint64)


def seam_case(bc_len, heavy=50, light=1):
    """-> (whitelist, barcodes, expected low bits of the midpoints, midpoints).  For every PAIR of whitelist_np.ballot_specs two
    midpoints, the first with `heavy` exact reads on its first candidate and `light` on the second, the other the reverse: the
    winner is on either side of the 63 / 64 seam of the two ballots.  At 32 bases also midpoints next to the all-ones key, whose
    counter lives outside the table: as winner (neighbour 0, 63, 64, 95 of the midpoint) and as loser (2, 65, 66, 93), its rival in
    the other ballot or the same.  The barcodes are the exact reads and one read of every midpoint, shuffled."""
    rng = np.random.default_rng([0x1B00800, bc_len])
    pairs = [s for s in wnp.ballot_specs(bc_len) if len(s) == 2]
    wl, bc, mids, low = [], [], [], []

    def plant(c, first, second, first_wins):
        wl.extend([first, second])
        bc.extend([first] * (heavy if first_wins else light) + [second] * (light if first_wins else heavy))
        mids.append(c)
        low.append(first if first_wins else second)

    centres = iter(int(c) for c in wnp.random_codes(rng, bc_len, 2 * len(pairs)))
    for j1, j2 in pairs:
        for first_wins in (True, False):
            c = next(centres)
            plant(c, wnp.neighbour(c, j1), wnp.neighbour(c, j2), first_wins)
    if bc_len == 32:   # all ones has ONE counter: `heavy` reads; where it wins its rival has `light` reads, where it loses 60 x heavy.
        # The rivals sit at bases of their own (none shared, none a base at which a midpoint differs from all ones), so no
        # midpoint is a neighbour of another one's rival.
        bc.extend([wnp.FREE] * heavy)
        for j, j2, ones_wins in ((0, 3 * 30, True), (63, 3 * 5 + 1, True), (64, 3 * 28, True), (95, 3 * 2, True),
                                 (2, 3 * 29 + 1, False), (65, 3 * 7, False), (66, 3 * 27 + 2, False), (93, 3 * 10 + 1, False)):
            c = wnp.neighbour(wnp.FREE, j)                      # neighbour j of c is all ones again
            rival = wnp.neighbour(c, j2)
            wl.extend([wnp.FREE, rival])
            bc.extend([rival] * (light if ones_wins else 60 * heavy))
            mids.append(c)
            low.append(wnp.FREE if ones_wins else rival)
    mids_a = np.array(mids, np.uint64)
    allbc = np.concatenate([np.array(bc, np.uint64), mids_a])
    return np.array(wl, np.uint64), rng.permutation(allbc), np.array(low, np.uint64), mids_a
