"""The numpy statement of the count matrix (include/ibu_hip.h: ibu_records_swap_umi_index, ibu_pair_counts,
ibu_count_matrix), written from the header comment alone.  Test infrastructure: the product never imports it.

w0, w1, w2 are the three 64-bit words of a record in storage order.  swap: {w0, w1, w2} -> {w0, w2, w1}.  An entry of
pair_counts is a maximal run of consecutive records with equal (w0, w1): its two words, its length, and the number of
positions in it whose w2 differs from the record before (the first record of a run counts).  count_matrix: swap, sort by
the three words, pair_counts — one entry per (barcode, index) pair with its reads and its distinct UMIs."""
import numpy as np

REC = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("index", "<u8")])


def _words(recs):
    return np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)


def swap(recs):
    """Record i of the result = {w0, w2, w1} of record i of recs."""
    return np.ascontiguousarray(_words(recs)[:, [0, 2, 1]]).view(REC).reshape(-1)


def pair_counts(recs):
    """-> (first, second, records_per_pair, distinct_third), one entry per maximal run of equal (w0, w1), in input order.
    No sorting inside: for unsorted input this is the run-length encoding."""
    w = _words(recs)
    n = len(w)
    if n == 0:
        e = np.empty(0, np.uint64)
        return e, e.copy(), e.copy(), e.copy()
    pair_head = np.ones(n, bool)
    pair_head[1:] = (w[1:, 0] != w[:-1, 0]) | (w[1:, 1] != w[:-1, 1])
    triple_head = pair_head.copy()
    triple_head[1:] |= w[1:, 2] != w[:-1, 2]
    starts = np.flatnonzero(pair_head)
    ends = np.append(starts[1:], n)
    rank = np.concatenate([[0], np.cumsum(triple_head)])          # triple heads in front of row i
    return (w[starts, 0].copy(), w[starts, 1].copy(), (ends - starts).astype(np.uint64), (rank[ends] - rank[starts]).astype(np.uint64))


def sort_records(recs):
    """Ascending by (w0, w1, w2) as unsigned 64-bit words."""
    return np.sort(np.ascontiguousarray(recs).view(REC).reshape(-1), order=["barcode", "umi", "index"])


def count_matrix(recs):
    """-> (barcodes, indices, reads, umis) ascending by (barcode, index), and the swapped-and-sorted records they were read off."""
    s = sort_records(swap(recs))
    return pair_counts(s), s


def brute_force_matrix(recs):
    """The same with a Python dict of sets: {(barcode, index): (reads, distinct umis)} in ascending key order."""
    reads, umis = {}, {}
    for b, u, i in _words(recs).tolist():
        reads[(b, i)] = reads.get((b, i), 0) + 1
        umis.setdefault((b, i), set()).add(u)
    keys = sorted(reads)
    return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64),
            np.array([reads[k] for k in keys], np.uint64), np.array([len(umis[k]) for k in keys], np.uint64))


def make_records(rng, n, bc_len, n_barcodes, n_indices, n_umis, high_bit=True):
    """n records over n_barcodes x n_indices x n_umis values, shuffled.  Barcodes are bc_len-base codes (full 64-bit words at 32
    bases); with high_bit the UMI and index values carry bit 63 on half of their alphabet, so unsigned order matters."""
    m = (1 << (2 * bc_len)) - 1
    bcs = (rng.integers(0, 1 << 62, n_barcodes, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, n_barcodes, dtype=np.uint64)) & np.uint64(m)
    umis = rng.integers(0, 1 << 24, n_umis, dtype=np.uint64)
    idxs = np.arange(n_indices, dtype=np.uint64)
    if high_bit:
        umis[::2] |= np.uint64(1 << 63)
        idxs[::2] |= np.uint64(1 << 63)
    r = np.empty(n, REC)
    r["barcode"] = bcs[rng.integers(0, n_barcodes, n)]
    r["umi"] = umis[rng.integers(0, n_umis, n)]
    r["index"] = idxs[(rng.random(n) ** 3 * n_indices).astype(np.int64)]   # skewed: the high indices are rare, so some pairs have one read
    return r


# ---- dense, unequal per-segment head counts beyond 1024 segments (the scan of the per-segment counters, ibu_k_runs_scan) --------
SEG = 8192                                                       # runs_walk.hpp: kSegRecs
STASH_HEADS = 32                                                 # runs_walk.hpp: kStashHeads
STASH_SEGMENTS = (3, 4, 6, 100, 102, 104, 106, 108, 253, 255, 256, 257, 259, 400, 401, 402, 406, 511, 512, 513, 640, 642, 644, 646, 767, 768,
                  769, 899, 900, 902, 1019, 1020, 1021, 1023, 1024, 1025, 1027, 1028, 1029, 1030)


def dense_runs(n, head, stash_segments=STASH_SEGMENTS):
    """Sorted records with (w0, w1) runs of 1 - 7 records in a fixed pseudo-random pattern, about half of them beginning a barcode
    and a new third word on two rows in five besides: the heads of a segment differ from its neighbours' at every level.  In the
    tiled segments named (first row head + 8192 (j - 1)) the barcodes are long instead: j % 29 barcode heads, none where that is 0."""
    rng = np.random.default_rng(0xC0F00)
    starts = np.cumsum(rng.integers(1, 8, n // 2))
    assert starts[-1] >= n
    h2 = np.zeros(n, bool)
    h2[0] = True
    h2[starts[starts < n]] = True
    h1 = h2 & (rng.random(n) < 0.5)
    h1[0] = True
    h3 = h2 | (rng.random(n) < 0.4)
    for j in stash_segments:
        a = head + SEG * (j - 1)
        assert 0 < a and a + SEG <= n
        h1[a:a + SEG] = False
        at = a + 100 + 277 * np.arange(j % 29)
        h1[at] = h2[at] = h3[at] = True
    r = np.zeros(n, REC)
    w = r.view(np.uint64).reshape(-1, 3)
    w[:, 0], w[:, 1], w[:, 2] = np.cumsum(h1), np.cumsum(h2), np.cumsum(h3)
    return r


def barcode_counts(recs):
    """-> (barcodes, counts, unique_umis), one entry per maximal run of equal w0 in input order: the run's length and the
    positions in it whose w1 differs from the record before (the first counts)."""
    w = _words(recs)
    n = len(w)
    head = np.ones(n, bool)
    head[1:] = w[1:, 0] != w[:-1, 0]
    ranked = head.copy()
    ranked[1:] |= w[1:, 1] != w[:-1, 1]
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    rank = np.concatenate([[0], np.cumsum(ranked)])
    return w[starts, 0].copy(), (ends - starts).astype(np.uint64), (rank[ends] - rank[starts]).astype(np.uint64)
