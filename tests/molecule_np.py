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


# ---- candidate-level layouts: the seams of the verdict blocks and of the scan over their summaries ----------------------------
MOL_BLOCK = 1024                                                 # k_molecules.hip: kMolBlock, candidates per verdict workgroup
SEAM_BLOCKS = (1, 2, 4, 255, 256, 257, 512, 768, 1023, 1024, 1025, 1028)   # thread, wave and round boundaries of the chains scan, in blocks
BLOCK_SIZES = (MOL_BLOCK * 1024, MOL_BLOCK * 1024 + 1, MOL_BLOCK * 1031 + 7)
HEAD_LAST_D = (1, 2, 1023, 1024, 1025)
WIN5 = ("win_trail", "win_mid", "win_lead", "tie_trail_lead", "all_tied")
WIN7 = ("win_trail", "win_before", "win_after", "win_lead", "tie_trail_lead", "tie_seam", "all_tied")
LONG = (250, 1029)                                               # one molecule from the middle of block 250 to the middle of block 1029
LONG_VARIANTS = ("win_head", "win_wave1", "win_before_round", "win_after_round", "win_lead", "tie_trail_lead", "tie_round_seam",
                 "tie_far", "all_tied")


def lay_candidates(reads, mol_head):
    """Sorted records from a candidate table: reads[c] = the length of candidate c, mol_head[c] = candidate c begins a molecule.
    w0 = the molecule's number (from 1), w2 = the candidate's number inside its molecule: distinct per candidate, ascending."""
    reads, mol_head = np.asarray(reads, np.int64), np.asarray(mol_head, bool)
    assert reads.shape == mol_head.shape and reads.ndim == 1 and (reads >= 1).all() and (len(reads) == 0 or mol_head[0])
    c = np.arange(len(reads), dtype=np.int64)
    first = np.maximum.accumulate(np.where(mol_head, c, 0))
    r = np.zeros(int(reads.sum()), REC)
    w = r.view(np.uint64).reshape(-1, 3)
    w[:, 0], w[:, 1], w[:, 2] = np.repeat(np.cumsum(mol_head), reads), 7, np.repeat(c - first, reads)
    return r


def _verdicts(a, b, twos):
    """What the rule gives a molecule of candidates a .. b - 1 with one read each but two on `twos`: [(candidate, class, class
    under tie_first)] for its first, its last and the candidates named."""
    at = sorted({a, b - 1, *twos})
    if len(twos) == 1 or b - a == 1:
        top = twos[0] if twos else a
        return [(c, KEPT if c == top else MINOR, KEPT if c == top else MINOR) for c in at]
    first = min(twos) if twos else a
    return [(c, TIED, KEPT if c == first else MINOR) for c in at]


def _piece(lo, hi, heads, twos, head_checks, molecules):
    classes = [v for a, b in molecules for v in _verdicts(a, b, [t for t in twos if a <= t < b])]
    return {"lo": lo, "hi": hi, "heads": sorted(heads), "twos": sorted(twos), "head_checks": head_checks, "classes": classes}


def seam_piece(spec, K, ncand):
    """The candidates a layout lays around block boundary B = 1024 K -> a piece (None where it does not fit ncand candidates):
    candidates lo .. hi - 1 have one read each but two on `twos` and begin a molecule exactly on `heads` (hi begins one too)."""
    B = MOL_BLOCK * K
    name = spec[0]
    if name == "ends_on_seam":                                   # (1, 1, 2) ends on B - 1: the winner is the block's last candidate
        end = min(B + 2, ncand)
        if B - 3 < 0 or B >= ncand:
            return None
        return _piece(B - 3, end, [B - 3, B], [B - 1], [(B - 1, False), (B, True)], [(B - 3, B), (B, end)])
    if name == "head_second":                                    # ends on B: the next block's lead piece is one candidate
        if B - 2 < 0 or B + 3 > ncand:
            return None
        return _piece(B - 2, B + 3, [B - 2, B + 1], [B if spec[1] else B - 1], [(B, False), (B + 1, True)], [(B - 2, B + 1), (B + 1, B + 3)])
    if name == "head_last":                                      # begins on the last candidate of block K - 1, d more candidates
        _, d, variant = spec
        a, b = B - 1, B + d
        if b > ncand:
            return None
        trail, mid, lead = a, B + (d - 1) // 2, b - 1
        twos = {"win_trail": [trail], "win_mid": [mid], "win_lead": [lead], "tie_trail_lead": [trail, lead], "all_tied": []}[variant]
        return _piece(a, b, [a], twos, [(a, True), (B, False), (b - 1, False)], [(a, b)])
    if name == "span":                                           # blocks K - 1, K, K + 1 without a molecule head
        a, b = B - 2 * MOL_BLOCK + 512, B + 2 * MOL_BLOCK + 512
        if a < 0 or b > ncand:
            return None
        trail, before, after, lead = a + 100, B - MOL_BLOCK + 300, B + 5, b - 7
        twos = {"win_trail": [trail], "win_before": [before], "win_after": [after], "win_lead": [lead], "tie_trail_lead": [trail, lead],
                "tie_seam": [B - 1, B], "all_tied": []}[spec[1]]
        return _piece(a, b, [a], twos, [(a, True)] + [(B + MOL_BLOCK * k, False) for k in (-1, 0, 1, 2)] + [(b - 1, False)], [(a, b)])
    assert name == "long"
    a, b = MOL_BLOCK * LONG[0] + 512, MOL_BLOCK * LONG[1] + 512
    if b > ncand:
        return None
    R = MOL_BLOCK * 1024                                         # the first candidate of the scan's second round
    twos = {"win_head": [a], "win_wave1": [MOL_BLOCK * 300 + 17], "win_before_round": [R - 1], "win_after_round": [R], "win_lead": [b - 1],
            "tie_trail_lead": [a + 1, b - 1], "tie_round_seam": [R - 1, R], "tie_far": [MOL_BLOCK * 600, MOL_BLOCK * 1026 + 1], "all_tied": []}[spec[1]]
    return _piece(a, b, [a], twos, [(a, True)] + [(MOL_BLOCK * k, False) for k in (251, 256, 512, 768, 1024, 1029)] + [(b - 1, False)], [(a, b)])


def seam_specs(i):
    """The layouts laid at the i-th seam block.  Every (block, d) of head_last occurs, the d that leave a block without a head
    twice; the place of the best rotates with i, so that every place occurs at thread, wave and round boundaries."""
    specs = [("ends_on_seam",), ("head_second", i % 2), ("head_last", 1, ("win_trail", "win_lead", "all_tied")[i % 3]), ("head_last", 2, WIN5[i % 5]),
             ("head_last", 1023, WIN5[i % 5]), ("head_last", 1024, WIN5[(i + 1) % 5]), ("head_last", 1024, WIN5[(i + 3) % 5]),
             ("head_last", 1025, WIN5[(i + 2) % 5]), ("head_last", 1025, WIN5[(i + 4) % 5])]
    spans = [WIN7[(2 * i + t) % 7] for t in (0, 1, 2)]
    if SEAM_BLOCKS[i] in (256, 1024) and "tie_seam" not in spans:
        spans.append("tie_seam")                                 # the tie across the wave seam and across the round seam
    specs += [("span", v) for v in spans]
    return specs[i % len(specs):] + specs[:i % len(specs)]


def seam_plan(ncand):
    """-> [[(K, spec), ...] per array]: every (K, spec) that fits ncand candidates laid once, the pieces of an array disjoint.
    Greedy and deterministic; the long molecule has arrays of its own."""
    pending = {K: [s for s in seam_specs(i) if seam_piece(s, K, ncand) is not None] for i, K in enumerate(SEAM_BLOCKS)}
    arrays = []
    while any(pending.values()):
        laid, end = [], 0
        for K in SEAM_BLOCKS:
            for s in pending[K]:
                if seam_piece(s, K, ncand)["lo"] >= end + 8:
                    laid.append((K, s))
                    end = seam_piece(s, K, ncand)["hi"]
                    pending[K].remove(s)
                    break
        arrays.append(laid)
    arrays += [[(LONG[1], ("long", v))] for v in LONG_VARIANTS if seam_piece(("long", v), LONG[1], ncand) is not None]
    return arrays


def seam_table(ncand, laid):
    """-> (reads, mol_head, pieces): short molecules of 1 - 5 candidates, one in sixteen candidates with two reads, and the pieces
    of `laid` over them."""
    rng = np.random.default_rng(0x30D00 + ncand)
    starts = np.cumsum(rng.integers(1, 6, ncand))
    mol_head = np.zeros(ncand, bool)
    mol_head[0] = True
    mol_head[starts[starts < ncand]] = True
    reads = 1 + (rng.random(ncand) < 1 / 16).astype(np.int64)
    pieces = [seam_piece(s, K, ncand) for K, s in laid]
    for p in pieces:
        reads[p["lo"]:p["hi"]] = 1
        reads[p["twos"]] = 2
        mol_head[p["lo"]:p["hi"]] = False
        mol_head[p["heads"]] = True
        if p["hi"] < ncand:
            mol_head[p["hi"]] = True
    return reads, mol_head, pieces


def check_seam_table(reads, mol_head, pieces, recs, want):
    """From the numpy side alone: the records round-trip to the table, every piece has its heads and non-heads on the candidates
    it is about, and the statement gives those candidates the classes the piece is about."""
    starts, mol = _runs(recs)
    rows = np.concatenate([[0], np.cumsum(reads)])
    assert len(starts) == len(reads) and (starts == rows[:-1]).all() and len(recs) == rows[-1]
    assert (mol == np.cumsum(mol_head) - 1).all()
    for p in pieces:
        for c, is_head in p["head_checks"]:
            assert bool(mol_head[c]) == is_head and (c == 0 or (mol[c] != mol[c - 1]) == is_head), (p, c)
        for c, plain, first in p["classes"]:
            assert (want[False][0][rows[c]:rows[c + 1]] == plain).all() and (want[True][0][rows[c]:rows[c + 1]] == first).all(), (p, c)
