"""One index per molecule on the device (ibu_classify_molecules): every comparison is byte for byte against the numpy statement
of the semantics in tests/molecule_np.py, the seven totals included; every call goes through the C ABI, and every buffer —
d_class at exactly n bytes too — is carved at its contract size out of an arena with guard zones (the pattern of
tests/test_gpu_count.py).  The records are compared after every call: they are never written."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import count_np as cnp
from tests import molecule_np as mnp
from tests.test_gpu_count import PATTERN, _arena, _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 63, 127, 128, 129, 255, 2559, 2561, 5121, 100_003, 1_000_003]
SEG, TILE = 8192, 128                                            # k_aggregate.hip: records per segment / per tile
SEAM_ROWS = [(SEG * k, d) for k in (1, 2, 12) for d in (-1, 0, 1)] + [(TILE * k, d) for k in (3, 63, 65) for d in (-1, 0, 1)]
NS = SIZES + [s + d for s, d in SEAM_ROWS]
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
SHAPES = ["scaled", "own_molecule", "one_candidate", "two_candidates", "n_candidates", "seam_2_3", "seam_3_2", "seam_3_2_3", "seam_molecules"]
GRID = list(itertools.product(NS, SKEWS, SHAPES))
assert len(set(NS)) == len(NS) == 31 and len(GRID) == 558
GARBAGE = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _classify(ia, ctx, d, n, flags, d_class, want_counts=True, stream=None):
    """One call through the C ABI -> the seven totals as a dict (None without counts)."""
    from ibu_amd import _lib
    c = _lib.CMoleculeCounts(*[GARBAGE] * 8)
    ia._check(ia.lib.ibu_classify_molecules(ctx._c, _p(d), n, flags, _p(d_class), C.byref(c) if want_counts else None, stream))
    if not want_counts:
        return None
    assert c.reserved == 0
    return {k: int(getattr(c, k)) for k in mnp.TOTALS}


def _lay(w, a, reads, key):
    """Rows a .. of w become one molecule (key, 0) whose candidates have these reads."""
    row = a
    for j, r in enumerate(reads):
        w[row:row + r, 0], w[row:row + r, 1], w[row:row + r, 2] = key, 0, 10 + j
        row += r


def _seam(shape, n, head, d):
    """Ordinary three-record molecules (reads 2, 1) and, at every seam row s + d + head that fits, a molecule laid so that the
    boundary between two of its candidates (seam_molecules: between two molecules) is that row."""
    r = np.zeros(n, cnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    w[:, 0], w[:, 1], w[:, 2] = i // np.uint64(3), 7, (i % np.uint64(3)) // np.uint64(2)
    laid = []
    for k, s in enumerate(sorted({s for s, _ in SEAM_ROWS})):
        row = s + d + head
        big = (1 << 40) + 2 * k
        if shape == "seam_2_3":
            a, reads = row - 2, [(2, 3)]
        elif shape == "seam_3_2":
            a, reads = row - 3, [(3, 2)]
        elif shape == "seam_3_2_3":                              # the tie's two halves on either side: the first or the second boundary on the row
            a, reads = (row - 3, [(3, 2, 3)]) if k % 2 == 0 else (row - 5, [(3, 2, 3)])
        else:
            a, reads = row - 3, [(1, 2), (2, 1)]
        if a < 0 or a + sum(sum(x) for x in reads) > n:
            continue
        for j, x in enumerate(reads):
            _lay(w, a, x, big + j)
            a += sum(x)
        laid.append(row)
    mol_head = np.ones(n, bool)
    mol_head[1:] = (w[1:, 0] != w[:-1, 0]) | (w[1:, 1] != w[:-1, 1])
    cand_head = mol_head.copy()
    cand_head[1:] |= w[1:, 2] != w[:-1, 2]
    for row in laid:
        assert cand_head[row] and mol_head[row] == (shape == "seam_molecules"), (shape, row)
    return r, laid


@functools.lru_cache(maxsize=6)
def _shape(shape, n, skew, d=0):
    """-> (records, {tie_first: (class bytes, totals)})."""
    r = np.zeros(n, cnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    if shape == "scaled":
        r = mnp.make_sorted(mnp.SEED + n, n)
    elif shape == "own_molecule":
        w[:, 0], w[:, 1], w[:, 2] = i >> np.uint64(1), i & np.uint64(1), 9
    elif shape == "one_candidate":
        w[:, 0], w[:, 1], w[:, 2] = 5, 6, 7
    elif shape == "two_candidates":                              # floor(n/2) and ceil(n/2) reads: a tie when n is even
        w[:, 0], w[:, 1], w[:, 2] = 5, 6, (i >= np.uint64(n // 2)).astype(np.uint64)
    elif shape == "n_candidates":                                # one molecule of n candidates: the long-molecule path
        w[:, 0], w[:, 1], w[:, 2] = 5, 6, i
    else:
        r = _seam(shape, n, min(skew // 8, n), d)[0]
    want = {f: mnp.classify(r, f) for f in (False, True)}
    t = want[False][1]
    if shape == "own_molecule":
        assert t["candidates"] == t["molecules"] == n and t["reads_kept"] == n
    elif shape == "one_candidate":
        assert t["candidates"] == min(n, 1) and t["reads_kept"] == n
    elif shape == "two_candidates" and n >= 2:
        assert (t["tied"], t["resolved"]) == ((1, 0) if n % 2 == 0 else (0, 1))
        assert n % 2 == 0 or want[False][0].tolist() == [1] * (n // 2) + [0] * (n - n // 2), "the winner is the last candidate"
    elif shape == "n_candidates" and n >= 2:
        assert t["candidates"] == n and t["reads_tied"] == n and want[True][0].tolist() == [0] + [1] * (n - 1)
    elif shape == "scaled" and n >= 63:
        assert all((want[False][0] == c).any() for c in (0, 1, 2)), "all three classes"
    return r, want


def _check_case(ia, ctx, recs, want, n, skew):
    ar = _arena(ia, ctx, 24 * n, n, n)
    try:
        d = ar.carve(24 * n, skew)
        if n:
            d.upload(recs)
        for tie_first, cls_skew in ((False, 0), (True, 3)):       # (with the one record a skewed base peels: word and byte stores of the fill)
            d_class = ar.carve(n, cls_skew)
            got = _classify(ia, ctx, d, n, ia.MOLECULES_TIE_FIRST if tie_first else 0, d_class)
            ar.check(f"classify_molecules tie_first={tie_first}")
            cls, tot = want[tie_first]
            assert got == tot, (got, tot)
            if n:
                have = d_class.download(np.uint8, n)
                bad = np.flatnonzero(have != cls)
                assert bad.size == 0, f"{bad.size} class bytes differ, first at row {int(bad[0])}: {int(have[bad[0]])} for {int(cls[bad[0]])}"
        assert n == 0 or d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
    finally:
        ar.free()


@pytest.mark.parametrize("n,skew,shape", GRID)
def test_classify_matches_numpy(ia, ctx, n, skew, shape):
    for d in ((-1, 0, 1) if shape.startswith("seam") and n > TILE * 3 else (0,)):
        recs, want = _shape(shape, n, skew, d)
        _check_case(ia, ctx, recs, want, n, skew)


def test_every_seam_row_is_laid_at_the_largest_size():
    for shape in SHAPES[5:]:
        for d in (-1, 0, 1):
            laid = _seam(shape, 100_003, 0, d)[1]
            assert laid == [s + d for s in sorted({s for s, _ in SEAM_ROWS})], (shape, d, laid)


def test_unsorted_input_is_the_run_level_answer(ia, ctx):
    n = 100_003
    recs = mnp.make_sorted(mnp.SEED + n, n)[np.random.default_rng(0x30A00).permutation(n)]
    want = {f: mnp.classify(recs, f) for f in (False, True)}
    assert want[False][1]["molecules"] > 2 * mnp.classify(cnp.sort_records(recs))[1]["molecules"] and want[False][1]["tied"] > 0
    _check_case(ia, ctx, recs, want, n, 8)


def test_forms_of_the_call(ia, ctx):
    n = 100_003
    recs, want = _shape("scaled", n, 0)
    cls, tot = want[False]
    ar = _arena(ia, ctx, 24 * n, n, n)
    other = ia.Context(0)
    try:
        d, d_class = ar.carve(24 * n, 8), ar.carve(n, 1)
        d.upload(recs)
        pattern = np.full(n, PATTERN, np.uint8).tobytes()
        # an unknown flag bit, too many records, bad pointers: refused before anything is touched
        for flags in (2, 3, 1 << 31):
            with pytest.raises(ia.IbuError) as ei:
                _classify(ia, ctx, d, n, flags, d_class)
            assert ei.value.kind == "InvalidArg"
        for args in ((d, 1 << 40), (None, 1), (ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 24), 1)):
            with pytest.raises(ia.IbuError) as ei:
                _classify(ia, ctx, args[0], args[1], 0, d_class)
            assert ei.value.kind == "InvalidArg"
        ar.check("refused calls")
        assert d_class.download(np.uint8, n).tobytes() == pattern, "a refused call writes nothing"
        # totals only
        assert _classify(ia, ctx, d, n, 0, None) == tot
        ar.check("counts only")
        assert d_class.download(np.uint8, n).tobytes() == pattern
        # classes only, twice on one context (the scratch is reused), then on a stream of another context
        for _ in range(2):
            assert _classify(ia, ctx, d, n, 0, d_class, want_counts=False) is None
            ar.check("classes only")
            assert d_class.download(np.uint8, n).tobytes() == cls.tobytes()
        assert _classify(ia, ctx, d, n, 1, d_class) == want[True][1]
        assert d_class.download(np.uint8, n).tobytes() == want[True][0].tobytes()
        assert _classify(ia, ctx, d, n, 0, d_class, stream=other.stream) == tot
        other.synchronize(other.stream)
        ar.check("another stream")
        assert d_class.download(np.uint8, n).tobytes() == cls.tobytes()
        assert _classify(ia, ctx, None, 0, 0, None) == dict.fromkeys(mnp.TOTALS, 0)
        # the Python wrapper
        buf, counts = ctx.classify_molecules(d, n)
        ctx.synchronize()
        assert counts == ia.MoleculeCounts(**tot) and buf.download(np.uint8, n).tobytes() == cls.tobytes()
        buf.free()
        assert ctx.classify_molecules(d, n, d_class=False, tie_first=True) == (None, ia.MoleculeCounts(**want[True][1]))
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        other.close()
        ar.free()


def _matrix_of(entries):
    return {(int(b), int(i)): [int(r), int(u)] for b, i, r, u in zip(*entries)}


@pytest.mark.parametrize("n", [2561, 100_003])
@pytest.mark.parametrize("tie_first", [False, True])
def test_sort_classify_select_count_matrix(ia, ctx, n, tie_first):
    rng = np.random.default_rng(0x30B00 + n)
    recs = cnp.make_records(rng, n, 16, n_barcodes=max(2, n // 24), n_indices=3, n_umis=4)
    want = mnp.resolved_matrix(recs, tie_first)
    molecules = len({(b, u) for b, u, _ in recs.tolist()})
    assert 0 < sum(v[1] for v in want.values()) <= molecules and (tie_first or sum(v[1] for v in want.values()) < molecules), "ties are dropped"
    d, tmp, d_class = ctx.upload(recs), ctx.alloc(24 * n), ctx.alloc(n)
    ctx.sort_records(d, tmp, n)
    _, counts = ctx.classify_molecules(d, n, d_class, tie_first=tie_first)
    out, k = ctx.select_records(d, d_class, n, 1 << ia.MOLECULE_KEPT)
    assert k == counts.reads_kept == sum(v[0] for v in want.values())
    ctx.synchronize()
    kept = out.download(cnp.REC, k)
    assert kept.tobytes() == cnp.sort_records(kept).tobytes(), "still sorted"
    mol = ctx.pair_counts(out, k)
    assert (mol[3] == 1).all() and len(mol[0]) == sum(v[1] for v in want.values()), "one index per molecule"
    assert _matrix_of(ctx.count_matrix(out, tmp, k)) == want
    for b in (d, tmp, d_class, out):
        b.free()


def test_count_file_resolve(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    n, bc_len = 20_000, 16
    recs = cnp.make_records(np.random.default_rng(0x30C00), n, bc_len, n_barcodes=n // 24, n_indices=3, n_umis=4, high_bit=False)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    text = lambda c: "".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(bc_len))
    want = mnp.resolved_matrix(recs)
    r = subprocess.run([str(exe), "--resolve", str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    matrix = [l for l in r.stdout.splitlines() if not l.startswith("#")]
    assert matrix == [f"{text(b)}\t{i}\t{v[1]}\t{v[0]}" for (b, i), v in sorted(want.items())]
    tot = mnp.classify(cnp.sort_records(recs))[1]
    assert (f"{n} records: molecules {tot['molecules']}, candidates {tot['candidates']}, resolved {tot['resolved']}, tied {tot['tied']}; "
            f"reads kept {tot['reads_kept']}, minor {tot['reads_minor']}, tied {tot['reads_tied']}") in r.stderr
