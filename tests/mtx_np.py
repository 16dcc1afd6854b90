"""The numpy / Python statement of the matrix export (include/ibu_hip.h: ibu_matrix_rows, ibu_matrix_market_body), written from the
header comment alone, and a reader of the directory Context.write_matrix_market leaves.  Test infrastructure: the product never
imports it.

matrix_rows: a ROW is a maximal run of consecutive entries with equal first[k] (A, B, A is three rows).  body: line k is
dec(a[k] + add_a) ' ' dec(b[k] + add_b) ' ' dec(c[k]) '\\n', the sums modulo 2^64, dec the shortest decimal form."""
import os

import numpy as np

M64 = (1 << 64) - 1
BANNER = "%%MatrixMarket matrix coordinate integer general"


def matrix_rows(first):
    """-> (row_of_entry, keys, ptr), u64 arrays of n, n_rows and n_rows + 1 words; ptr[n_rows] = n.  No entries: ptr = [0]."""
    first = np.ascontiguousarray(first, np.uint64)
    n = len(first)
    if n == 0:
        e = np.empty(0, np.uint64)
        return e, e.copy(), np.zeros(1, np.uint64)
    head = np.ones(n, bool)
    head[1:] = first[1:] != first[:-1]
    starts = np.flatnonzero(head)
    return (np.cumsum(head) - 1).astype(np.uint64), first[starts].copy(), np.append(starts, n).astype(np.uint64)


def body(a, b, c, add_a, add_b):
    """-> (bytes, maxima): the text, formatted with Python integers, and the largest printed value of each column (zeros for no
    entries)."""
    cols = [[(int(v) + add) & M64 for v in col] for col, add in ((a, add_a), (b, add_b), (c, 0))]
    text = "".join(f"{x} {y} {z}\n" for x, y, z in zip(*cols)).encode()
    return text, tuple(max(col, default=0) for col in cols)


def read_directory(directory):
    """matrix.mtx + barcodes.tsv + features.tsv -> (n_features, barcodes, feature ids, [(barcode text, feature number, value)]) with the
    triples in file order and the feature number 0-based."""
    with open(os.path.join(directory, "matrix.mtx")) as f:
        assert f.readline() == BANNER + "\n"
        n_features, n_rows, nnz = (int(x) for x in f.readline().split())
        lines = f.read().splitlines()
    barcodes = open(os.path.join(directory, "barcodes.tsv")).read().splitlines()
    features = [l.split("\t") for l in open(os.path.join(directory, "features.tsv")).read().splitlines()]
    assert len(lines) == nnz and len(barcodes) == n_rows and len(features) == n_features
    assert all(len(f) == 3 and f[2] == "Gene Expression" for f in features)
    coo = []
    for l in lines:
        i, j, v = (int(x) for x in l.split(" "))
        assert 1 <= i <= n_features and 1 <= j <= n_rows
        coo.append((barcodes[j - 1], i - 1, v))
    return n_features, barcodes, [f[0] for f in features], coo
