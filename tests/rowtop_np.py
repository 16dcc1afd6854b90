"""The numpy / Python statement of ibu_matrix_row_top and ibu_assign_rows, written from the comment in include/ibu_hip.h alone: the
checker of tests/test_gpu_rowtop.py, itself checked against a per-row loop in tests/test_rowtop_host.py.  Python integers wherever 64
bits could overflow (the row sum modulo 2^64, the 128-bit products of the share test).  The product never imports this."""
import numpy as np

NO_KEY = (1 << 64) - 1
ROW_ASSIGNED, ROW_NONE, ROW_MIXED = 0, 1, 2
M64 = (1 << 64) - 1
U = np.uint64


def bitmap(values, n_bits):
    """The bitmap ibu_barcode_metrics takes: bit v is bit v & 63 of u64 word v >> 6; (n_bits + 63) // 64 words, at least one."""
    words = [0] * max((n_bits + 63) // 64, 1)
    for v in values:
        assert 0 <= v < n_bits
        words[v >> 6] |= 1 << (v & 63)
    return np.array(words, dtype=np.uint64)


def takes_part(second, set_words=None, set_bits=0):
    """Entry k takes part iff there is no set, or second[k] < set_bits and bit second[k] of the bitmap is set."""
    second = np.asarray(second, dtype=np.uint64)
    if set_words is None:
        assert set_bits == 0
        return np.ones(len(second), bool)
    below = second < U(set_bits) if set_bits <= M64 else np.ones(len(second), bool)
    word = np.where(below, second >> U(6), U(0)).astype(np.int64)   # a key of set_bits or more is never looked up
    bit = (np.asarray(set_words, dtype=np.uint64)[word] >> (second & U(63))) & U(1)
    return below & (bit != 0)


def row_starts(first):
    """The index of every row's first entry: a row is a maximal run of consecutive entries with equal first[k]."""
    first = np.asarray(first, dtype=np.uint64)
    if len(first) == 0:
        return np.empty(0, np.int64)
    return np.concatenate([[0], np.flatnonzero(first[1:] != first[:-1]) + 1]).astype(np.int64)


def row_top(first, second, values, set_words=None, set_bits=0):
    """-> (top_key, top_value, next_value, row_sum, row_entries), one u64 per row."""
    first, second, values = (np.asarray(a, dtype=np.uint64) for a in (first, second, values))
    n = len(first)
    starts = row_starts(first)
    r = len(starts)
    if r == 0:
        return tuple(np.empty(0, np.uint64) for _ in range(5))
    part = takes_part(second, set_words, set_bits)
    row = np.repeat(np.arange(r), np.diff(np.concatenate([starts, [n]])))
    v = np.where(part, values, U(0))
    entries = np.add.reduceat(part.astype(np.uint64), starts)
    top_value = np.maximum.reduceat(v, starts)
    # the FIRST entry, in entry order, that takes part and holds the largest value
    at = np.flatnonzero(part & (values == top_value[row]))
    rows_with, where = np.unique(row[at], return_index=True)
    top_at = at[where]
    top_key = np.full(r, NO_KEY, np.uint64)
    top_key[rows_with] = second[top_at]
    others = v.copy()
    others[top_at] = 0                                           # the largest value among the OTHER entries that take part
    next_value = np.maximum.reduceat(others, starts)
    if int(v.max()) * n <= M64:                                  # no sum can reach 2^64: u64 arithmetic is exact
        row_sum = np.add.reduceat(v, starts)
    else:                                                        # Python integers, then modulo 2^64
        row_sum = np.array([int(s) & M64 for s in np.add.reduceat(v.astype(object), starts)], dtype=np.uint64)
    return top_key, top_value, next_value, row_sum, entries


def assign(top_value, next_value, row_sum, min_value, num, den):
    """-> (class bytes, {"rows", "assigned", "none", "mixed"}): NONE if top < max(min_value, 1); ASSIGNED if top > next and
    top * den >= num * sum (exact; num == 0: no share test); MIXED otherwise."""
    assert den >= 1 and num <= den
    floor = max(int(min_value), 1)
    cls = np.empty(len(top_value), np.uint8)
    for k, (t, nx, s) in enumerate(zip(np.asarray(top_value).tolist(), np.asarray(next_value).tolist(), np.asarray(row_sum).tolist())):
        if t < floor:
            cls[k] = ROW_NONE
        elif t > nx and (num == 0 or t * den >= num * s):
            cls[k] = ROW_ASSIGNED
        else:
            cls[k] = ROW_MIXED
    counts = {"rows": len(cls), "assigned": int((cls == ROW_ASSIGNED).sum()), "none": int((cls == ROW_NONE).sum()),
              "mixed": int((cls == ROW_MIXED).sum())}
    return cls, counts
