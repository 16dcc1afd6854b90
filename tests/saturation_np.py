"""The numpy statement of ibu_subsample_class and ibu_saturation_curve (include/ibu_hip.h), written from the header comment alone.
Test infrastructure: the product never imports it.

splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
z ^ (z >> 31), all modulo 2^64.  The number of a read: u(row) = splitmix64(splitmix64(seed) + first_row + row).  A read is kept at
threshold t iff u(row) < t or t is all ones.  A point of the curve: the kept reads, and the maximal runs of equal w0 / of equal
(w0, w1) with at least one kept read — a run is kept iff the smallest u among its reads is."""
import numpy as np

from tests import count_np as cnp

REC = cnp.REC
KEPT, DROPPED = 0, 1
ONES = (1 << 64) - 1
MAX_POINTS = 32
FIELDS = ("threshold", "reads", "barcodes", "molecules")
_M64 = ONES


def splitmix64(z):
    """On a Python int or a uint64 array (wrapping)."""
    if isinstance(z, np.ndarray):
        with np.errstate(over="ignore"):
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def u(seed, first_row, n):
    """The numbers of rows 0 .. n - 1 as a uint64 array, in wrapping arithmetic."""
    base = (splitmix64(int(seed)) + int(first_row)) & _M64
    with np.errstate(over="ignore"):
        return splitmix64(np.uint64(base) + np.arange(n, dtype=np.uint64))


def kept(uu, t):
    return np.ones(len(uu), bool) if t == ONES else uu < np.uint64(t)


def subsample_class(n, seed, first_row, t):
    """-> (class bytes, the number kept)."""
    k = kept(u(seed, first_row, n), t)
    return np.where(k, KEPT, DROPPED).astype(np.uint8), int(k.sum())


def sample_threshold(fraction):
    from fractions import Fraction
    return ONES if fraction >= 1 else int(Fraction(fraction) * (1 << 64))


def _heads(recs):
    w = cnp._words(recs)
    n = len(w)
    h1 = np.ones(n, bool)
    h1[1:] = w[1:, 0] != w[:-1, 0]
    h2 = h1.copy()
    h2[1:] |= w[1:, 1] != w[:-1, 1]
    return h1, h2


def saturation_curve(recs, seed, first_row, thresholds):
    """-> [(threshold, reads, barcodes, molecules)] — the run minima by np.minimum.reduceat over the head positions."""
    n = len(recs)
    if n == 0:
        return [(int(t), 0, 0, 0) for t in thresholds]
    uu = u(seed, first_row, n)
    h1, h2 = _heads(recs)
    m1 = np.minimum.reduceat(uu, np.flatnonzero(h1))
    m2 = np.minimum.reduceat(uu, np.flatnonzero(h2))
    return [(int(t), int(kept(uu, t).sum()), int(kept(m1, t).sum()), int(kept(m2, t).sum())) for t in thresholds]


def brute_force(recs, seed, first_row, thresholds):
    """The same in plain Python loops over the runs: a run counts iff any of its reads is kept."""
    rows = cnp._words(recs).tolist()
    base = (splitmix64(seed) + first_row) & _M64
    nums = [splitmix64((base + r) & _M64) for r in range(len(rows))]
    out = []
    for t in thresholds:
        keep = [t == ONES or x < t for x in nums]
        reads = sum(keep)
        barcodes = molecules = 0
        r = 0
        while r < len(rows):
            e = r
            while e < len(rows) and rows[e][0] == rows[r][0]:
                e += 1
            barcodes += any(keep[r:e])
            q = r
            while q < e:
                p = q
                while p < e and rows[p][1] == rows[q][1]:
                    p += 1
                molecules += any(keep[q:p])
                q = p
            r = e
        out.append((int(t), reads, barcodes, molecules))
    return out
