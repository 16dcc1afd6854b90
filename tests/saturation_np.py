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
    return saturation_curve_from(u(seed, first_row, len(recs)), recs, thresholds)


def head_positions(recs):
    """-> (rows that begin a barcode, rows that begin a molecule)."""
    h1, h2 = _heads(recs)
    return np.flatnonzero(h1), np.flatnonzero(h2)


def saturation_curve_from(uu, recs, thresholds, heads=None):
    """The same from the reads' numbers themselves, uu[row] = u(row): a caller that asks about many first_row on one seed slices
    them out of one sequence.  heads: head_positions(recs), for a caller that asks often about the same records."""
    n = len(recs)
    assert len(uu) == n
    if n == 0:
        return [(int(t), 0, 0, 0) for t in thresholds]
    p1, p2 = heads if heads is not None else head_positions(recs)
    m1 = np.minimum.reduceat(uu, p1)
    m2 = np.minimum.reduceat(uu, p2)
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


# ---- layouts for the scan over the segments' summaries (ibu_k_saturation_stitch) ----------------------------------------------
SEG = 8192                                                       # runs_walk.hpp: kSegRecs


def seg_first_row(head, j):
    """The first row of tiled segment j >= 1 when `head` rows are peeled in front (segment 0)."""
    return head + (j - 1) * SEG


def recs_of_heads(h1, h2):
    """Sorted records whose barcodes begin on h1 and whose molecules begin on h2 (which includes h1)."""
    assert h1[0] and not (h1 & ~h2).any()
    r = np.zeros(len(h1), REC)
    w = r.view(np.uint64).reshape(-1, 3)
    w[:, 0], w[:, 1], w[:, 2] = np.cumsum(h1), np.cumsum(h2), 1
    return r


def stitch_mixed(n, seed=0x32900):
    """Barcodes of 0.3 to 5 segments, molecules of 10 records to 1.5 segments (log-uniform), neither a multiple of the other:
    segments without a head, with one and with several, at both depths."""
    rng = np.random.default_rng(seed)
    h1, h2 = np.zeros(n, bool), np.zeros(n, bool)
    for h, lo, hi in ((h1, 0.3 * SEG, 5 * SEG), (h2, 10, 1.5 * SEG)):
        lengths = np.exp(rng.uniform(np.log(lo), np.log(hi), int(4 * n / lo ** 0.5 / hi ** 0.5) + 16)).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(lengths)])
        assert starts[-1] >= n
        h[starts[starts < n]] = True
    return recs_of_heads(h1, h1 | h2)


def stitch_runs(n, head, layout, seams, long=(200, 1029)):
    """Molecules of three records, barcodes of six, and runs at both depths laid over them -> (records, [(J, rows)]).
    through: for every seam J a run whose head is row 5 of segment J - 2 and which ends 100 rows into segment J + 1 (segments
    J - 1 and J have no head); rows = just behind the head, the last row of J - 1, the first of J, the last row of the run.
    head_on_seam: the same with a head on the first row of segment J; rows = the last row of J - 1 and the first of J.
    long: one run from segment long[0] to segment long[1]; rows = its two ends, and the last row in front of and the first row of
    segments 256, 512, 768 (the waves of the scan), 1024 (its second round) and 1025."""
    i = np.arange(n)
    h2 = i % 3 == 0
    h1 = i % 6 == 0
    rows = []

    def lay(a, b):
        for h in (h1, h2):
            h[a:b] = False
            h[a] = h[b] = True

    F = lambda j: seg_first_row(head, j)
    if layout == "long":
        a, b = F(long[0]) + 5, F(long[1]) + 100
        lay(a, b)
        rows.append((1024, [a + 1] + [F(j) + e for j in (256, 512, 768, 1024, 1025) for e in (-1, 0)] + [b - 1]))
    else:
        for J in seams:
            a, b = F(J - 2) + 5, F(J + 1) + 100
            lay(a, b)
            if layout == "head_on_seam":
                h1[F(J)] = h2[F(J)] = True
                rows.append((J, [F(J) - 1, F(J)]))
            else:
                assert layout == "through"
                rows.append((J, [a + 1, F(J) - 1, F(J), b - 1]))
    return recs_of_heads(h1, h2), rows
