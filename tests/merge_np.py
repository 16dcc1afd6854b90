"""The merge of sorted records (ibu_merge_sorted, ibu_merge_sorted_runs) stated in numpy — the statement the GPU tests compare
against byte for byte.  The reference has no merge; the semantics are this library's (include/ibu_hip.h).  Order: the three 64-bit
words of a record in storage order, unsigned; among equal records those of `a` come first, within each input the order is kept."""
import numpy as np

from tests.count_np import REC


def _words(recs):
    return np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)


def merge(a, b):
    """-> (out, source): a stable sort of the tagged concatenation on (w0, w1, w2, source); source[p] = 0 (from a) or 1 (from b)."""
    w = np.concatenate([_words(a), _words(b)])
    tag = np.concatenate([np.zeros(len(a), np.uint8), np.ones(len(b), np.uint8)])
    order = np.lexsort((tag, w[:, 2], w[:, 1], w[:, 0]))        # the last key is the primary one; lexsort is stable
    return np.ascontiguousarray(w[order]).view(REC).reshape(-1), tag[order]


def merge_runs(recs, lengths):
    """Consecutive sorted runs of these lengths -> all records sorted: pairwise merges of neighbouring runs, level by level."""
    recs = np.ascontiguousarray(recs).view(REC).reshape(-1)
    assert sum(lengths) == len(recs)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    runs = [recs[starts[k]:starts[k + 1]] for k in range(len(lengths))]
    while len(runs) > 1:
        runs = [merge(runs[k], runs[k + 1])[0] if k + 1 < len(runs) else runs[k] for k in range(0, len(runs), 2)]
    return runs[0] if runs else recs


def _le(x, y):
    """x <= y for two records as rows of three u64 words."""
    return tuple(int(v) for v in x) <= tuple(int(v) for v in y)


def diagonal(a, b, d):
    """The number of a-records among the first d records of merge(a, b): the binary search of include/ibu_hip.h."""
    wa, wb = _words(a), _words(b)
    lo, hi = max(0, d - len(wb)), min(d, len(wa))
    while lo < hi:
        mid = (lo + hi) // 2
        if _le(wa[mid], wb[d - 1 - mid]):
            lo = mid + 1
        else:
            hi = mid
    return lo
