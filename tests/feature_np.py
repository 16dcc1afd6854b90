"""The numpy statement of ibu_feature_metrics and ibu_filter_features, written from the text of include/ibu_hip.h alone.

Write w0, w1, w2 for the three words of a record.  A PAIR is a maximal run of consecutive records with equal (w0, w1), a TRIPLE one
with equal (w0, w1, w2).  The FEATURE of a record is the value f of its word feature_word (1 or 2).  For every f < n_features:
reads[f] = the records with that feature, umis[f] = the triples with it, cells[f] = the pairs with it (feature_word 1 only).  A record
with f >= n_features enters no column.  totals = (sum of reads, sum of umis, sum of cells, records out of range).  The filter gives
feature f the first verdict that applies — LOW (a count below its minimum), HIGH (a count above its non-zero maximum), else PASS —
and every record the verdict of its feature, UNKNOWN where f >= n_features."""
import numpy as np

REC = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("index", "<u8")])
PASS, LOW, HIGH, UNKNOWN = 0, 1, 2, 3
COLUMNS = ("reads", "umis", "cells")
LIMITS = ("min_reads", "max_reads", "min_umis", "max_umis", "min_cells", "max_cells")
TOTALS = ("features_by_class", "reads_by_class", "reserved")


def _words(recs):
    return np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)


def feature_metrics(recs, n_features, feature_word=1, into=None):
    """-> ((reads, umis, cells), totals): u64 columns of n_features entries (cells is None for feature_word 2) and the four totals of
    this call.  into: a (reads, umis, cells) triple the counts are added on top of (IBU_FEATURE_ACCUMULATE)."""
    assert feature_word in (1, 2) and 1 <= n_features <= 1 << 32
    w = _words(recs)
    n = len(w)
    pair = np.ones(n, bool)
    pair[1:] = (w[1:, 0] != w[:-1, 0]) | (w[1:, 1] != w[:-1, 1])
    triple = pair.copy()
    triple[1:] |= w[1:, 2] != w[:-1, 2]
    f = w[:, feature_word]
    ok = f < np.uint64(n_features)                               # compared as 64-bit values: 2^32 + k is not feature k
    fi = f[ok].astype(np.int64)
    col = lambda heads: np.bincount(fi if heads is None else fi[heads[ok]], minlength=n_features).astype(np.uint64)
    cols = [col(None), col(triple), col(pair) if feature_word == 1 else None]
    totals = (int(cols[0].sum()), int(cols[1].sum()), int(cols[2].sum()) if feature_word == 1 else 0, int(n - ok.sum()))
    if into is not None:
        cols = [None if c is None else c + np.asarray(o, np.uint64) for c, o in zip(cols, into)]
    return tuple(cols), totals


def limits(**kw):
    """A limits dict, every field 0 unless given."""
    assert set(kw) <= set(LIMITS)
    return dict(dict.fromkeys(LIMITS, 0), **kw)


def verdicts(table, lim, n_features):
    """One verdict byte per feature from the (reads, umis, cells) columns; a column that is None counts as 0 and must have no limit."""
    low, high = np.zeros(n_features, bool), np.zeros(n_features, bool)
    for col, name in zip(table, COLUMNS):
        lo, hi = lim["min_" + name], lim["max_" + name]
        if col is None:
            assert lo == 0 and hi == 0, "a NULL column whose limits are not both 0 is refused"
            continue
        assert len(col) == n_features
        low |= col < np.uint64(lo)
        if hi:
            high |= col > np.uint64(hi)
    return np.where(low, LOW, np.where(high, HIGH, PASS)).astype(np.uint8)


def record_features(recs, n_features, feature_word):
    """-> (which records have a feature below n_features, the features of those records)."""
    assert feature_word in (1, 2)
    f = _words(recs)[:, feature_word]
    ok = f < np.uint64(n_features)
    return ok, f[ok].astype(np.int64)


def filter_features(recs, n_features, feature_word, table, lim, features=None):
    """-> (verdict bytes per feature, class bytes per record, the totals as a dict of tuples).  features: what record_features gave
    for these records, for a caller that filters them under several limits."""
    v = verdicts(table, lim, n_features)
    ok, fi = features or record_features(recs, n_features, feature_word)
    cls = np.full(len(ok), UNKNOWN, np.uint8)
    cls[ok] = v[fi]
    tot = {"features_by_class": tuple(np.bincount(v, minlength=3).tolist()), "reads_by_class": tuple(np.bincount(cls, minlength=4).tolist()),
           "reserved": 0}
    return v, cls, tot


def brute_force(recs, n_features, feature_word, lim=None):
    """The same with Python dicts and one loop over the records -> (reads, umis, cells as lists, totals), and with limits also
    (verdicts, classes, totals of the filter) made from those very columns."""
    rows = [tuple(int(x) for x in r) for r in _words(recs)]
    reads, umis, cells, out = {}, {}, {}, 0
    for k, r in enumerate(rows):
        f = r[feature_word]
        if f >= n_features:
            out += 1
            continue
        prev = rows[k - 1] if k else None
        reads[f] = reads.get(f, 0) + 1
        if prev is None or prev != r:
            umis[f] = umis.get(f, 0) + 1
        if feature_word == 1 and (prev is None or prev[:2] != r[:2]):
            cells[f] = cells.get(f, 0) + 1
    col = lambda d: [d.get(f, 0) for f in range(n_features)]
    table = (col(reads), col(umis), col(cells) if feature_word == 1 else None)
    totals = (sum(reads.values()), sum(umis.values()), sum(cells.values()), out)
    if lim is None:
        return table, totals
    verdict = []
    for f in range(n_features):
        counts = {"reads": table[0][f], "umis": table[1][f], "cells": table[2][f] if table[2] is not None else 0}
        v = PASS
        if any(lim["max_" + c] and counts[c] > lim["max_" + c] for c in COLUMNS):
            v = HIGH
        if any(counts[c] < lim["min_" + c] for c in COLUMNS):
            v = LOW
        verdict.append(v)
    cls = [verdict[r[feature_word]] if r[feature_word] < n_features else UNKNOWN for r in rows]
    tot = {"features_by_class": tuple(verdict.count(c) for c in range(3)), "reads_by_class": tuple(cls.count(c) for c in range(4)), "reserved": 0}
    return table, totals, (np.array(verdict, np.uint8), np.array(cls, np.uint8), tot)
