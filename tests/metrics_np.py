"""The numpy statement of ibu_barcode_metrics and ibu_filter_barcodes, written from the text of include/ibu_hip.h alone.

Write w0, w1, w2 for the three words of a record.  A BARCODE is a maximal run of consecutive records with equal w0, a PAIR one with
equal (w0, w1), a TRIPLE one with equal (w0, w1, w2).  A record is IN THE SET iff the value v of its word set_word (1 or 2) is below
set_bits and bit v & 63 of bitmap word v >> 6 is set.  Per barcode: its records, the pairs and triples that begin in it, its records
in the set, its triples in the set.  The filter gives every record the class of its barcode, the first that applies: LOW (a count
below its minimum), HIGH (a count above its non-zero maximum), SET (set_x * set_den > set_num * x), else PASS."""
import numpy as np

REC = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("index", "<u8")])
PASS, LOW, HIGH, SET = 0, 1, 2, 3
COLUMNS = ("barcodes", "reads", "pairs", "triples", "set_reads", "set_triples")
LIMITS = ("min_reads", "max_reads", "min_pairs", "max_pairs", "min_triples", "max_triples", "set_num", "set_den", "set_of", "reserved")
TOTALS = ("barcodes", "barcodes_by_class", "reads_by_class", "triples_passed", "set_triples_passed", "reserved")


def bitmap(values, n_bits):
    """u64 words of a set of n_bits bits with the bits `values` (each below n_bits) set; at least one word."""
    words = np.zeros(max((n_bits + 63) // 64, 1), np.uint64)
    for v in values:
        assert 0 <= v < n_bits
        words[v >> 6] |= np.uint64(1 << (v & 63))
    return words


def in_set(values, words, set_bits):
    """One bool per value (u64 array)."""
    values = np.asarray(values, np.uint64)
    out = np.zeros(len(values), bool)
    if set_bits == 0 or len(values) == 0:
        return out
    ok = values < np.uint64(set_bits)
    v = values[ok]
    out[ok] = ((words[(v >> np.uint64(6)).astype(np.int64)] >> (v & np.uint64(63))) & np.uint64(1)).astype(bool)
    return out


def barcode_metrics(recs, words=None, set_bits=0, set_word=1):
    """-> (barcodes, reads, pairs, triples, set_reads, set_triples), u64 arrays, a row per barcode in input order."""
    assert set_word in (1, 2) and set_bits <= 1 << 32
    n = len(recs)
    if n == 0:
        return tuple(np.empty(0, np.uint64) for _ in COLUMNS)
    w = np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)
    h0 = np.ones(n, bool)
    h0[1:] = w[1:, 0] != w[:-1, 0]
    h1 = h0.copy()
    h1[1:] |= w[1:, 1] != w[:-1, 1]
    h2 = h1.copy()
    h2[1:] |= w[1:, 2] != w[:-1, 2]
    member = in_set(w[:, set_word], words, set_bits)
    first = np.flatnonzero(h0)
    sums = lambda x: np.add.reduceat(x.astype(np.uint64), first)
    return (w[first, 0].copy(), sums(np.ones(n, bool)), sums(h1), sums(h2), sums(member), sums(member & h2))


def limits(**kw):
    """A limits dict, every field 0 unless given."""
    assert set(kw) <= set(LIMITS)
    return dict(dict.fromkeys(LIMITS, 0), **kw)


def verdicts(table, lim):
    """One class per barcode of a barcode_metrics table.  (u64 products: with counts below 2^40 and set_num <= set_den < 2^24 none
    overflows — brute_force does the same in Python integers.)"""
    u = lambda name: np.uint64(lim[name])
    reads, pairs, triples, set_reads, set_triples = table[1:]
    assert lim["set_den"] < 1 << 24 and (len(reads) == 0 or int(reads.max()) < 1 << 40)
    x, set_x = (triples, set_triples) if lim["set_of"] else (reads, set_reads)
    low = (reads < u("min_reads")) | (pairs < u("min_pairs")) | (triples < u("min_triples"))
    high = np.zeros(len(reads), bool)
    for col, name in ((reads, "max_reads"), (pairs, "max_pairs"), (triples, "max_triples")):
        if lim[name]:
            high |= col > u(name)
    over = (set_x * u("set_den") > u("set_num") * x) if lim["set_den"] else np.zeros(len(reads), bool)
    return np.where(low, LOW, np.where(high, HIGH, np.where(over, SET, PASS))).astype(np.uint8)


def filter_barcodes(recs, words, set_bits, set_word, lim, table=None):
    """-> (one class byte per record, the totals as a dict: the two by_class entries are 4-tuples)."""
    assert lim["set_of"] in (0, 1) and lim["set_num"] <= lim["set_den"] < 1 << 24
    table = barcode_metrics(recs, words, set_bits, set_word) if table is None else table
    v = verdicts(table, lim)
    reads = table[1].astype(np.int64)
    cls = np.repeat(v, reads)
    tot = {"barcodes": len(v),
           "barcodes_by_class": tuple(int((v == c).sum()) for c in range(4)),
           "reads_by_class": tuple(int(reads[v == c].sum()) for c in range(4)),
           "triples_passed": int(table[3][v == PASS].sum()),
           "set_triples_passed": int(table[5][v == PASS].sum()),
           "reserved": 0}
    return cls, tot


def brute_force(recs, words, set_bits, set_word, lim=None):
    """The same, one barcode at a time with Python sets and loops -> (table as lists, classes, totals)."""
    rows = [tuple(int(x) for x in r) for r in np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)]
    has = lambda v: v < set_bits and (int(words[v // 64]) >> (v % 64)) & 1 == 1
    table, k = [], 0
    while k < len(rows):
        j = k
        while j < len(rows) and rows[j][0] == rows[k][0]:
            j += 1
        run = rows[k:j]
        pairs = 1 + sum(1 for a, b in zip(run, run[1:]) if a[:2] != b[:2])
        heads = [run[0]] + [b for a, b in zip(run, run[1:]) if a != b]
        table.append((rows[k][0], j - k, pairs, len(heads), sum(1 for r in run if has(r[set_word])), sum(1 for r in heads if has(r[set_word]))))
        k = j
    if lim is None:
        return table
    cls, tot = [], {"barcodes": len(table), "barcodes_by_class": [0] * 4, "reads_by_class": [0] * 4, "triples_passed": 0, "set_triples_passed": 0,
                    "reserved": 0}
    for _, reads, pairs, triples, set_reads, set_triples in table:
        x, set_x = (triples, set_triples) if lim["set_of"] else (reads, set_reads)
        c = PASS
        if lim["set_den"] and set_x * lim["set_den"] > lim["set_num"] * x:
            c = SET
        if any(mx and val > mx for mx, val in ((lim["max_reads"], reads), (lim["max_pairs"], pairs), (lim["max_triples"], triples))):
            c = HIGH
        if reads < lim["min_reads"] or pairs < lim["min_pairs"] or triples < lim["min_triples"]:
            c = LOW
        cls += [c] * reads
        tot["barcodes_by_class"][c] += 1
        tot["reads_by_class"][c] += reads
        if c == PASS:
            tot["triples_passed"] += triples
            tot["set_triples_passed"] += set_triples
    tot["barcodes_by_class"], tot["reads_by_class"] = tuple(tot["barcodes_by_class"]), tuple(tot["reads_by_class"])
    return table, np.array(cls, np.uint8), tot
