"""The numpy statement of ibu_classify_molecules (include/ibu_hip.h), written from the header comment alone.  Test
infrastructure: the product never imports it.

w0, w1, w2 are the three 64-bit words of a record in storage order.  A molecule is a maximal run of consecutive records with
equal (w0, w1), a candidate a maximal run with equal (w0, w1, w2); a candidate's reads is its length, a molecule's best the
largest reads among its candidates.  Class 0 (kept): the only candidate of its molecule at best.  Class 1 (minor): another
candidate of a molecule with exactly one at best.  Class 2 (tied): every record of a molecule with two or more at best.
tie_first: in a tied molecule the first candidate at best is class 0 and the rest of the molecule class 1."""
import numpy as np

from tests import count_np as cnp

REC = cnp.REC
KEPT, MINOR, TIED = 0, 1, 2
TOTALS = ("molecules", "candidates", "resolved", "tied", "reads_kept", "reads_minor", "reads_tied")


def _words(recs):
    return np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 3)


def _runs(recs):
    """-> (first row of every candidate, the molecule number of every candidate)."""
    w = _words(recs)
    n = len(w)
    mol_head = np.ones(n, bool)
    mol_head[1:] = (w[1:, 0] != w[:-1, 0]) | (w[1:, 1] != w[:-1, 1])
    cand_head = mol_head.copy()
    cand_head[1:] |= w[1:, 2] != w[:-1, 2]
    starts = np.flatnonzero(cand_head)
    return starts, np.cumsum(mol_head)[starts] - 1


def classify(recs, tie_first=False):
    """-> (class bytes, one per record; the seven totals as a dict)."""
    n = len(recs)
    if n == 0:
        return np.zeros(0, np.uint8), dict.fromkeys(TOTALS, 0)
    starts, mol = _runs(recs)
    reads = np.diff(np.append(starts, n))
    n_mol = int(mol[-1]) + 1
    best = np.zeros(n_mol, np.int64)
    np.maximum.at(best, mol, reads)
    at_best = reads == best[mol]
    n_at_best = np.bincount(mol, weights=at_best, minlength=n_mol).astype(np.int64)
    n_cand = np.bincount(mol, minlength=n_mol)
    cand = np.arange(len(starts))
    first_at_best = np.full(n_mol, len(starts), np.int64)
    np.minimum.at(first_at_best, mol[at_best], cand[at_best])
    tied_mol = n_at_best >= 2
    if tie_first:
        cls = np.where(cand == first_at_best[mol], KEPT, MINOR)
    else:
        cls = np.where(tied_mol[mol], TIED, np.where(at_best, KEPT, MINOR))
    per_record = np.repeat(cls.astype(np.uint8), reads)
    totals = {"molecules": n_mol, "candidates": len(starts), "resolved": int(((n_cand >= 2) & (n_at_best == 1)).sum()),
              "tied": int(tied_mol.sum()), "reads_kept": int((per_record == KEPT).sum()), "reads_minor": int((per_record == MINOR).sum()),
              "reads_tied": int((per_record == TIED).sum())}
    return per_record, totals


def molecule_runs(recs):
    """[[(w2, reads), ...] per molecule] in input order: the runs as they stand (Python ints)."""
    out, prev = [], None
    for b, u, i in _words(recs).tolist():
        if prev is None or (b, u) != prev[:2]:
            out.append([[i, 1]])
        elif i != prev[2]:
            out[-1].append([i, 1])
        else:
            out[-1][-1][1] += 1
        prev = (b, u, i)
    return out


def brute_force(recs, tie_first=False):
    """The same with Python lists over the runs."""
    cls = []
    t = dict.fromkeys(TOTALS, 0)
    for cands in molecule_runs(recs):
        reads = [r for _, r in cands]
        best = max(reads)
        top = [k for k, r in enumerate(reads) if r == best]
        t["molecules"] += 1
        t["candidates"] += len(cands)
        t["resolved"] += len(cands) >= 2 and len(top) == 1
        t["tied"] += len(top) >= 2
        for k, r in enumerate(reads):
            if len(top) >= 2 and not tie_first:
                c = TIED
            else:
                c = KEPT if k == top[0] else MINOR
            cls += [c] * r
            t[("reads_kept", "reads_minor", "reads_tied")[c]] += r
    return np.array(cls, np.uint8), {k: int(v) for k, v in t.items()}


SEED = 0x30700   # make_sorted(SEED + n, n) has all three classes at every size the tests use from 63 records on (checked there)


def make_sorted(seed, n):
    """Sorted records whose alphabet grows with n, so that every class occurs at every size (about two thirds kept, a quarter
    minor, a tenth tied)."""
    rng = np.random.default_rng(seed)
    return cnp.sort_records(cnp.make_records(rng, n, 16, n_barcodes=max(2, n // 24), n_indices=3, n_umis=4))


def recs_of(rows):
    r = np.zeros(len(rows), REC)
    for k, (b, u, i) in enumerate(rows):
        r[k] = (b, u, i)
    return r


def resolved_matrix(recs, tie_first=False):
    """{(barcode, index): [reads, molecules]} of the kept records, built with dicts from the sorted records: every (barcode, umi)
    molecule counts once, under the index it was seen with strictly most often (ties: dropped, or the smallest index)."""
    per = {}
    for b, u, i in _words(recs).tolist():
        d = per.setdefault((b, u), {})
        d[i] = d.get(i, 0) + 1
    out = {}
    for (b, u), d in per.items():
        best = max(d.values())
        top = sorted(i for i, r in d.items() if r == best)
        if len(top) >= 2 and not tie_first:
            continue
        e = out.setdefault((b, top[0]), [0, 0])
        e[0] += best
        e[1] += 1
    return out
