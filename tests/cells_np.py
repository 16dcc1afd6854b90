"""The numpy statement of ibu_call_cells (include/ibu_hip.h), written from the header comment alone.  Test infrastructure: the
product never imports it.

w0, w1 are the first two 64-bit words of a record in storage order.  A barcode is a maximal run of consecutive records with equal
w0; its reads is the length of the run, its umis the number of positions in the run whose w1 differs from the record before it
(the first position counts).  The metric is umis, or reads under by_reads.  With the B metrics in descending order m(1) >= ... >=
m(B), one threshold T decides — a barcode is a cell (class 0) iff metric >= T, background (class 1) otherwise:
  MIN     T = param; baseline = 0
  TOP     T = m(min(K, B)); baseline = 0
  ORDMAG  E' = min(E, B), baseline = m(E' // 100 + 1), T = (baseline + 9) // 10"""
import numpy as np

from tests import count_np as cnp

REC = cnp.REC
CELL, BACKGROUND = 0, 1
MIN, TOP, ORDMAG = 0, 1, 2
BY_READS = 1
TOTALS = ("barcodes", "cells", "threshold", "baseline", "reads_cells", "reads_background", "umis_cells", "umis_background")


def _words(recs):
    return np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)


def barcode_table(recs):
    """-> (first row, reads, umis) of every barcode run, in input order (int64 arrays)."""
    w = _words(recs)
    n = len(w)
    head = np.ones(n, bool)
    head[1:] = w[1:, 0] != w[:-1, 0]
    ranked = head.copy()
    ranked[1:] |= w[1:, 1] != w[:-1, 1]
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    rank = np.concatenate([[0], np.cumsum(ranked)])
    return starts, ends - starts, rank[ends] - rank[starts]


def threshold(metric, mode, param):
    """-> (T, baseline) for the metrics of B >= 1 barcodes (any order)."""
    if mode == MIN:
        return int(param), 0
    desc = np.sort(np.asarray(metric, np.int64))[::-1]
    b = len(desc)
    if mode == TOP:
        return int(desc[min(param, b) - 1]), 0
    baseline = int(desc[min(param, b) // 100])                # m(E' // 100 + 1), one-based
    return (baseline + 9) // 10, baseline


def call_cells(recs, mode, param, by_reads=False, table=None):
    """-> (class bytes, one per record; the eight totals as a dict).  table: barcode_table(recs), for a caller that asks often."""
    n = len(recs)
    if n == 0:
        t = dict.fromkeys(TOTALS, 0)
        t["threshold"] = int(param) if mode == MIN else 0
        return np.zeros(0, np.uint8), t
    _, reads, umis = table if table is not None else barcode_table(recs)
    metric = reads if by_reads else umis
    T, baseline = threshold(metric, mode, param)
    cell = metric >= T if T < (1 << 63) else np.zeros(len(metric), bool)    # (no metric reaches 2^63; numpy would compare as floats)
    cls = np.where(cell, CELL, BACKGROUND).astype(np.uint8)
    totals = {"barcodes": len(reads), "cells": int(cell.sum()), "threshold": T, "baseline": baseline,
              "reads_cells": int(reads[cell].sum()), "reads_background": int(reads[~cell].sum()),
              "umis_cells": int(umis[cell].sum()), "umis_background": int(umis[~cell].sum())}
    return np.repeat(cls, reads), totals


def brute_force(recs, mode, param, by_reads=False):
    """The same, deliberately naive: Python lists over the runs, the metric list sorted with sorted(), the definitions applied
    literally with one-based ranks."""
    runs, prev = [], None                                      # [reads, umis] per barcode
    for b, u, _ in _words(recs).tolist():
        if prev is None or b != prev[0]:
            runs.append([1, 1])
        else:
            runs[-1][0] += 1
            runs[-1][1] += u != prev[1]
        prev = (b, u)
    t = dict.fromkeys(TOTALS, 0)
    if not runs:
        t["threshold"] = param if mode == MIN else 0
        return np.zeros(0, np.uint8), t
    metric = [r[0] if by_reads else r[1] for r in runs]
    m = [None] + sorted(metric, reverse=True)                  # m[1] >= m[2] >= ... >= m[B]
    B = len(runs)
    if mode == MIN:
        T, baseline = param, 0
    elif mode == TOP:
        T, baseline = m[min(param, B)], 0
    else:
        e = min(param, B)
        baseline = m[e // 100 + 1]
        T = (baseline + 9) // 10
    cls = []
    t["barcodes"], t["threshold"], t["baseline"] = B, T, baseline
    for (reads, umis), x in zip(runs, metric):
        cell = x >= T
        cls += [CELL if cell else BACKGROUND] * reads
        t["cells"] += cell
        t["reads_cells" if cell else "reads_background"] += reads
        t["umis_cells" if cell else "umis_background"] += umis
    return np.array(cls, np.uint8), {k: int(v) for k, v in t.items()}


def recs_of_metrics(umis, reads_per_umi=1, first_barcode=1):
    """Sorted records: barcode k (ascending from first_barcode) has umis[k] UMIs of reads_per_umi records each."""
    umis = np.asarray(umis, np.int64)
    per = umis * reads_per_umi
    n = int(per.sum())
    r = np.zeros(n, REC)
    bc = np.repeat(np.arange(len(umis), dtype=np.uint64) + np.uint64(first_barcode), per)
    start = np.repeat(np.concatenate([[0], np.cumsum(per)[:-1]]), per)
    r["barcode"], r["umi"], r["index"] = bc, ((np.arange(n) - start) // reads_per_umi).astype(np.uint64), 3
    return r


def knee(rng, n_cells, n_background, cell_umis=(200, 400), reads_per_umi=1):
    """Sorted records with a knee: n_cells barcodes of hundreds of UMIs scattered among n_background barcodes of 1-3 UMIs."""
    umis = np.concatenate([rng.integers(cell_umis[0], cell_umis[1], n_cells), rng.integers(1, 4, n_background)])
    return recs_of_metrics(umis[rng.permutation(len(umis))], reads_per_umi)
