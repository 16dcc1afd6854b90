"""The numpy statement of barcode correction against a whitelist (include/ibu_hip.h, ibu_correct_barcodes), written from
the header comment alone.  Test infrastructure: the product never imports it.

A whitelist is a set of bc_len-base codes.  low = barcode & mask(2*bc_len); a neighbour of low is low ^ (x << 2i) for
i in [0, bc_len), x in {1, 2, 3}.  Classes: 0 exact (low in the whitelist), 1 corrected (not exact, exactly one
neighbour in it: the low bits become that neighbour), 2 ambiguous (not exact, two or more), 3 unmatched."""
import numpy as np

EXACT, CORRECTED, AMBIGUOUS, UNMATCHED = 0, 1, 2, 3
REC = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("index", "<u8")])


def mask(bc_len):
    return np.uint64((1 << (2 * bc_len)) - 1)


def _member(wl_sorted, keys):
    pos = np.searchsorted(wl_sorted, keys)
    pos[pos == len(wl_sorted)] = 0
    return wl_sorted[pos] == keys


def classify(barcodes, whitelist, bc_len, max_mismatches=1):
    """-> (class per barcode as uint8, the barcodes after correction as uint64)."""
    bc = np.ascontiguousarray(barcodes, dtype=np.uint64)
    wl = np.unique(np.asarray(whitelist, dtype=np.uint64))
    m = mask(bc_len)
    low = bc & m
    exact = _member(wl, low)
    cls = np.where(exact, EXACT, UNMATCHED).astype(np.uint8)
    out = bc.copy()
    if max_mismatches == 0:
        return cls, out
    miss = np.flatnonzero(~exact)
    lm = low[miss]
    hits = np.zeros(len(miss), np.int64)
    cand = np.zeros(len(miss), np.uint64)
    for i in range(bc_len):
        for x in (1, 2, 3):
            nb = lm ^ np.uint64(x << (2 * i))
            h = _member(wl, nb)
            cand = np.where(h & (hits == 0), nb, cand)
            hits += h
    cls[miss] = np.where(hits == 1, CORRECTED, np.where(hits >= 2, AMBIGUOUS, UNMATCHED)).astype(np.uint8)
    one = hits == 1
    out[miss[one]] = (bc[miss[one]] & ~m) | cand[one]
    return cls, out


def correct_records(recs, whitelist, bc_len, max_mismatches=1):
    """-> (records after correction, class bytes, {"exact", "corrected", "ambiguous", "unmatched"})."""
    recs = np.ascontiguousarray(recs).view(REC).reshape(-1)
    cls, bc = classify(recs["barcode"], whitelist, bc_len, max_mismatches)
    out = recs.copy()
    out["barcode"] = bc
    n = np.bincount(cls, minlength=4)
    return out, cls, {"exact": int(n[0]), "corrected": int(n[1]), "ambiguous": int(n[2]), "unmatched": int(n[3])}


def select(recs, cls, keep_mask):
    kept = [c for c in range(8) if (keep_mask >> c) & 1]
    return np.ascontiguousarray(recs).view(REC).reshape(-1)[np.isin(cls, kept)]


def brute_force(barcodes, whitelist, bc_len, max_mismatches=1):
    """The same with a Python set and a Hamming loop over the WHITELIST (no neighbour enumeration): small inputs only."""
    m = (1 << (2 * bc_len)) - 1
    wl = sorted({int(c) for c in whitelist})
    wls = set(wl)
    cls, out = [], []
    for b in (int(v) for v in barcodes):
        low = b & m
        if low in wls:
            cls.append(EXACT); out.append(b)
            continue
        near = []
        if max_mismatches:
            for c in wl:
                d = low ^ c
                pairs = (d | (d >> 1)) & 0x5555555555555555   # one bit per base that differs
                if pairs and pairs & (pairs - 1) == 0:
                    near.append(c)
        if len(near) == 1:
            cls.append(CORRECTED); out.append((b & ~m) | near[0])
        else:
            cls.append(AMBIGUOUS if near else UNMATCHED); out.append(b)
    return np.array(cls, np.uint8), np.array(out, np.uint64)


def make_case(rng, bc_len, w, n, junk=True, shares=(0.25, 0.25, 0.25, 0.25)):
    """A whitelist of w distinct random codes holding a planted pair at Hamming distance 2 (their midpoint is
    ambiguous), and n barcodes: `shares` of exact / one substitution / that midpoint / uniform random, shuffled; junk
    bits above 2*bc_len on half the barcodes where bc_len < 32.  -> (whitelist u64[w], barcodes u64[n])."""
    space = 4 ** bc_len
    if w > space:
        raise ValueError("4^bc_len < w")
    if space <= 1 << 20:
        wl = rng.permutation(space)[:w].astype(np.uint64)
    else:
        wl = np.empty(0, np.uint64)
        while len(wl) < w:
            more = rng.integers(0, 1 << 62, size=2 * w, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, size=2 * w, dtype=np.uint64)
            more &= mask(bc_len)
            wl = np.unique(np.concatenate([wl, more]))
        wl = rng.permutation(wl)[:w]
    mid = None
    if bc_len >= 2 and w >= 2:   # plant the pair: wl[1] = wl[0] with bases 0 and 1 substituted; the midpoint substitutes base 0 only
        a = int(wl[0])
        b = a ^ 0b0110
        midv = a ^ 0b0010
        rest = wl[2:][(wl[2:] != np.uint64(b)) & (wl[2:] != np.uint64(midv))]
        wl = np.concatenate([np.array([a, b], np.uint64), rest])
        mid = midv
    counts = [int(round(s * n)) for s in shares]
    counts[0] += n - sum(counts)
    exact = wl[rng.integers(0, len(wl), counts[0])]
    sub = wl[rng.integers(0, len(wl), counts[1])]
    sub = sub ^ (rng.integers(1, 4, counts[1], dtype=np.uint64) << (np.uint64(2) * rng.integers(0, bc_len, counts[1], dtype=np.uint64)))
    midp = np.full(counts[2], mid if mid is not None else int(wl[0]), np.uint64)
    rnd = (rng.integers(0, 1 << 62, size=counts[3], dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, size=counts[3], dtype=np.uint64)) & mask(bc_len)
    bc = rng.permutation(np.concatenate([exact, sub, midp, rnd]))
    if junk and bc_len < 32:
        j = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) << np.uint64(2 * bc_len)
        bc = np.where(rng.random(n) < 0.5, bc | j, bc)
    return wl, bc
