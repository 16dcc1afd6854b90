"""Cell calling on the device (ibu_call_cells; its selection alone through the test hook ibu_test_rank_select): every comparison is byte for byte against the numpy statement of the
semantics in tests/cells_np.py, the eight totals included; every call goes through the C ABI, and every buffer — d_class at
exactly n bytes too — is carved at its contract size out of an arena with guard zones (the pattern of tests/test_gpu_count.py).
The records are compared after every case: they are never written."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import cells_np as cnp
from tests import count_np
from tests.test_gpu_count import PATTERN, _arena, _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 63, 127, 128, 129, 255, 2559, 2561, 100_003, 1_000_003]
SEG, TILE = 8192, 128                                            # runs_walk.hpp: records per segment / per tile
SEAM_ROWS = [(SEG * k, d) for k in (1, 2, 12) for d in (-1, 0, 1)] + [(TILE * k, d) for k in (3, 63, 65) for d in (-1, 0, 1)]
NS = SIZES + [s + d for s, d in SEAM_ROWS]
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
SHAPES = ["own_barcode", "one_barcode", "knee", "seam", "two_values", "span"]
BIG = 1_000_003
# the grid: every size x skew x shape, but above 1e5 records only a handful (own_barcode and knee), and the run that spans three
# segments only where three segments exist
GRID = [(n, skew, shape) for n, skew, shape in itertools.product(NS, SKEWS, SHAPES)
        if (n < BIG or shape in ("own_barcode", "knee")) and (shape != "span" or n > 4 * SEG)]
assert len(set(NS)) == len(NS) == 30 and len(GRID) == 2 * (29 * 5 + 4 + 2), len(GRID)
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


def _call(ia, ctx, d, n, mode, param, flags, d_class, want_counts=True, stream=None):
    """One call through the C ABI -> the eight totals as a dict (None without counts)."""
    from ibu_amd import _lib
    c = _lib.CCellCounts(*[GARBAGE] * 8)
    ia._check(ia.lib.ibu_call_cells(ctx._c, _p(d), n, mode, param, flags, _p(d_class), C.byref(c) if want_counts else None, stream))
    if not want_counts:
        return None
    return {k: int(getattr(c, k)) for k in cnp.TOTALS}


def _seam(n, head, d):
    """Barcodes of three records and three UMIs and, at every seam row s + d + head that fits, a barcode of ten UMIs that ends
    just in front of the row and one of a single UMI (two records) that begins on it: under MIN 3 the two neighbours of the
    boundary are of different classes, and so are the cut barcodes around them."""
    r = np.zeros(n, cnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    w[:, 0], w[:, 1], w[:, 2] = i // np.uint64(3), i % np.uint64(3), 1
    laid = []
    for k, s in enumerate(sorted({s for s, _ in SEAM_ROWS})):
        row = s + d + head
        big = (1 << 40) + 2 * k
        if row - 10 < 0 or row + 2 > n:
            continue
        w[row - 10:row, 0], w[row - 10:row, 1] = big, np.arange(10, dtype=np.uint64)
        w[row:row + 2, 0], w[row:row + 2, 1] = big + 1, 5
        laid.append(row)
    return r, laid


def _span(n, head):
    """As above without the seams, and one barcode of two UMIs from just in front of the second segment to just behind the
    fourth: background by UMIs under MIN 3 between two cells, the only cell by reads under TOP 1."""
    r = np.zeros(n, cnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    w[:, 0], w[:, 1], w[:, 2] = i // np.uint64(3), i % np.uint64(3), 1
    a, b = head + SEG - 6, head + 4 * SEG + 9                     # both multiples of three away from `head`: whole neighbours
    a, b = a - (a % 3), b - (b % 3)
    w[a:b, 0], w[a:b, 1] = 1 << 41, (np.arange(b - a) >= SEG).astype(np.uint64)
    return r


@functools.lru_cache(maxsize=4)
def _shape(shape, n, skew, d=0):
    """-> (records, their barcode table)."""
    r = np.zeros(n, cnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    if shape == "own_barcode":                                   # B = n, every metric 1
        w[:, 0], w[:, 1], w[:, 2] = i, 7, 9
    elif shape == "one_barcode":
        w[:, 0], w[:, 1], w[:, 2] = 5, i >> np.uint64(1), 7
    elif shape == "knee":                                        # ~100 cells of hundreds of UMIs once n allows, 1-3 UMIs around them; cut to n records
        rng = np.random.default_rng(0x31300 + n)
        cells = min(100, n // 600 + 1)
        r = cnp.knee(rng, cells, n if n <= 1000 else n // 3 + 1, reads_per_umi=1 if n <= 1000 else 2)[:n].copy()
    elif shape == "two_values":                                  # reads 300 and 556 in turn (three and six UMIs): one middle digit apart
        reads = np.array([300 + 256 * (k & 1) for k in range(n // 300 + 2)])
        first = np.repeat(np.concatenate([[0], np.cumsum(reads)[:-1]]), reads)[:n]
        w[:, 0] = np.repeat(np.arange(len(reads), dtype=np.uint64), reads)[:n]
        w[:, 1], w[:, 2] = ((np.arange(n) - first) // 100).astype(np.uint64), 2
    elif shape == "seam":
        r = _seam(n, min(skew // 8, n), d)[0]
    else:
        r = _span(n, min(skew // 8, n))
    assert len(r) == n
    return r, cnp.barcode_table(r)


def _params(table, n):
    """(mode, param, by_reads) of the issue's list, deduplicated; above 1e5 records a handful."""
    out = []
    for by_reads in (False, True):
        metric = table[1] if by_reads else table[2]
        B = len(metric)
        mx, med = int(metric.max()), int(np.sort(metric)[B // 2])
        mins = [0, 1, med, mx, mx + 1]
        tops = [1, 2, B - 1, B, B + 1, 1 << 40]
        exps = [1, 99, 100, 101, B, 100 * B]
        if n >= BIG:
            mins, tops, exps = [med, mx], [2, B - 1], [100, B]
        out += [(cnp.MIN, p, by_reads) for p in dict.fromkeys(mins)]
        out += [(cnp.TOP, p, by_reads) for p in dict.fromkeys(tops) if p >= 1]
        out += [(cnp.ORDMAG, p, by_reads) for p in dict.fromkeys(exps) if p >= 1]
    return out


def _check_case(ia, ctx, recs, table, n, skew, params):
    ar = _arena(ia, ctx, 24 * n, n, n)
    try:
        d = ar.carve(24 * n, skew)
        d_classes = [ar.carve(n, 0), ar.carve(n, 3)]              # (with the one record a skewed base peels: word and byte stores of the fill)
        if n:
            d.upload(recs)
        for j, (mode, param, by_reads) in enumerate(params):
            d_class = d_classes[j & 1]
            got = _call(ia, ctx, d, n, mode, param, cnp.BY_READS if by_reads else 0, d_class)
            cls, tot = cnp.call_cells(recs, mode, param, by_reads, table)
            what = f"mode {mode} param {param} by_reads {by_reads}"
            assert got == tot, (what, got, tot)
            if n:
                have = d_class.download(np.uint8, n)
                bad = np.flatnonzero(have != cls)
                assert bad.size == 0, f"{what}: {bad.size} class bytes differ, first at row {int(bad[0])}: {int(have[bad[0]])} for {int(cls[bad[0]])}"
            if n < BIG or j == 0:
                ar.check(what)
        ar.check("call_cells")
        assert n == 0 or d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
    finally:
        ar.free()


@pytest.mark.parametrize("n,skew,shape", GRID)
def test_call_cells_matches_numpy(ia, ctx, n, skew, shape):
    for d in ((-1, 0, 1) if shape == "seam" and n > TILE * 3 else (0,)):
        recs, table = _shape(shape, n, skew, d)
        if n == 0:
            params = [(m, p, r) for m in (cnp.MIN, cnp.TOP, cnp.ORDMAG) for p in (0, 1, 7) for r in (False, True) if p or m == cnp.MIN]
        else:
            params = _params(table, n)
            if shape in ("seam", "span"):
                params.insert(0, (cnp.MIN, 3, False))
        _check_case(ia, ctx, recs, table, n, skew, params)


def test_the_shapes_have_what_they_claim():
    for d in (-1, 0, 1):
        recs, laid = _seam(100_003, 0, d)
        assert laid == [s + d for s in sorted({s for s, _ in SEAM_ROWS})], (d, laid)
        cls = cnp.call_cells(recs, cnp.MIN, 3)[0]
        assert all(cls[row - 1] == 0 and cls[row] == 1 for row in laid), "the two neighbours of every seam row are of different classes"
    recs, table = _shape("span", 100_003, 8)
    cls, tot = cnp.call_cells(recs, cnp.MIN, 3)
    long = int(np.argmax(table[1]))
    a, reads = int(table[0][long]), int(table[1][long])
    assert a < 1 + SEG and a + reads > 1 + 4 * SEG and cls[a] == 1 and cls[a - 1] == 0 and cls[a + reads] == 0, "three whole segments, between two cells"
    assert cnp.call_cells(recs, cnp.TOP, 1, True)[1]["cells"] == 1
    recs, table = _shape("two_values", 100_003, 0)
    assert set(table[1][:-1].tolist()) == {300, 556} and 300 ^ 556 == 0x300, "one middle digit"
    recs, table = _shape("knee", 100_003, 0)
    tot = cnp.call_cells(recs, cnp.ORDMAG, 100, False, table)[1]
    assert tot["cells"] == int((table[2] >= 100).sum()) >= 30 and tot["barcodes"] > 5_000 and 20 <= tot["threshold"] <= 40


# ---- the selection alone (ibu_test_rank_select: exported for tests, not part of the ABI): metric sets that make every digit pass decide, which records cannot reach -----------
def _metric_sets(rng, B):
    top = np.uint64(32)
    yield "all equal", np.full(B, 0x1234567890 >> 1, np.uint64)
    yield "bits 32-39 only", (rng.integers(0, 256, B, dtype=np.uint64) << top) | np.uint64(0x00ABCDEF12)
    yield "bits 0-7 only", rng.integers(0, 256, B, dtype=np.uint64) | np.uint64(0xFEDCBA9800)
    for digit in (1, 2, 3):
        yield f"two values, digit {digit}", np.uint64(0x0102030405) ^ (rng.integers(0, 2, B, dtype=np.uint64) << np.uint64(8 * digit + 3))
    yield "random below 2^40", rng.integers(0, 1 << 40, B, dtype=np.uint64)
    yield "small, many ties", rng.integers(1, 5, B, dtype=np.uint64)
    yield "the largest values", np.uint64((1 << 40) - 1) - rng.integers(0, 3, B, dtype=np.uint64)


@pytest.mark.parametrize("B", [1, 2, 63, 255, 257, 2049, 100_003, 1_000_003])
def test_rank_select_matches_a_sort(ia, ctx, B):
    from ibu_amd import _lib
    select = C.CDLL(_lib.SO_PATH).ibu_test_rank_select
    select.restype, select.argtypes = C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    rng = np.random.default_rng(0x31400 + B)
    ar = _arena(ia, ctx, 8 * B)
    try:
        d = ar.carve(8 * B, 8)
        for name, values in _metric_sets(rng, B):
            d.upload(values)
            desc = np.sort(values)[::-1]
            for rank in dict.fromkeys([1, 2, B // 100 + 1, B // 2, B - 1, B]):
                if not 1 <= rank <= B:
                    continue
                v = C.c_uint64(GARBAGE)
                ia._check(select(ctx._c, _p(d), B, rank, C.byref(v), None))
                assert v.value == int(desc[rank - 1]), (name, B, rank, hex(v.value), hex(int(desc[rank - 1])))
            assert d.download(np.uint64, B).tobytes() == values.tobytes(), "the values are read only"
        ar.check("rank_select")
        for n, rank, ptr in ((0, 1, d), (B, 0, d), (B, B + 1, d), (B, 1, None), (1 << 40, 1, d), (B, 1, ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 8))):
            v = C.c_uint64(GARBAGE)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(select(ctx._c, _p(ptr), n, rank, C.byref(v), None))
            assert ei.value.kind == "InvalidArg" and v.value == GARBAGE
    finally:
        ar.free()


def test_unsorted_input_is_the_run_level_answer(ia, ctx):
    n = 100_003
    recs = _shape("knee", n, 0)[0][np.random.default_rng(0x31500).permutation(n)]
    table = cnp.barcode_table(recs)
    assert len(table[0]) > 5 * len(_shape("knee", n, 0)[1][0])
    _check_case(ia, ctx, recs, table, n, 8, [(cnp.MIN, 2, False), (cnp.TOP, 1000, False), (cnp.ORDMAG, 5000, True)])


def test_forms_of_the_call(ia, ctx):
    n = 100_003
    recs, table = _shape("knee", n, 0)
    cls, tot = cnp.call_cells(recs, cnp.ORDMAG, 100, False, table)
    ar = _arena(ia, ctx, 24 * n, n, n)
    other = ia.Context(0)
    try:
        d, d_class = ar.carve(24 * n, 8), ar.carve(n, 1)
        d.upload(recs)
        pattern = np.full(n, PATTERN, np.uint8).tobytes()
        # every invalid argument is refused before anything is touched, the totals included
        from ibu_amd import _lib
        bad = [(d, n, 3, 1, 0), (d, n, 1 << 31, 1, 0), (d, n, 0, 1, 2), (d, n, 1, 5, 3), (d, n, 2, 5, 1 << 31), (d, n, 1, 0, 0), (d, n, 2, 0, 1),
               (d, 0, 1, 0, 0), (d, 0, 3, 1, 0), (d, 1 << 40, 0, 1, 0), (None, 1, 0, 1, 0), (ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 24), 1, 0, 1, 0)]
        for k, (buf, count, mode, param, flags) in enumerate(bad):
            c = _lib.CCellCounts(*[GARBAGE] * 8)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_call_cells(ctx._c, _p(buf), count, mode, param, flags, _p(d_class), C.byref(c), None))
            assert ei.value.kind == "InvalidArg", k
            assert all(getattr(c, f) == GARBAGE for f in cnp.TOTALS), (k, "the totals of a refused call are untouched")
        ar.check("refused calls")
        assert d_class.download(np.uint8, n).tobytes() == pattern, "a refused call writes nothing"
        # totals only
        assert _call(ia, ctx, d, n, cnp.ORDMAG, 100, 0, None) == tot
        ar.check("counts only")
        assert d_class.download(np.uint8, n).tobytes() == pattern
        # neither: nothing to see, nothing written
        assert _call(ia, ctx, d, n, cnp.TOP, 100, 0, None, want_counts=False) is None
        ctx.synchronize()
        ar.check("neither")
        assert d_class.download(np.uint8, n).tobytes() == pattern
        # classes only, twice on one context (the scratch is reused), then on a stream of another context
        for _ in range(2):
            assert _call(ia, ctx, d, n, cnp.ORDMAG, 100, 0, d_class, want_counts=False) is None
            ar.check("classes only")
            assert d_class.download(np.uint8, n).tobytes() == cls.tobytes()
        want = cnp.call_cells(recs, cnp.TOP, 7, True, table)
        assert _call(ia, ctx, d, n, cnp.TOP, 7, cnp.BY_READS, d_class, stream=other.stream) == want[1]
        other.synchronize(other.stream)
        ar.check("another stream")
        assert d_class.download(np.uint8, n).tobytes() == want[0].tobytes()
        assert _call(ia, ctx, None, 0, cnp.MIN, 9, 0, None) == dict(dict.fromkeys(cnp.TOTALS, 0), threshold=9)
        assert _call(ia, ctx, None, 0, cnp.ORDMAG, 9, 1, None) == dict.fromkeys(cnp.TOTALS, 0)
        # the Python wrapper
        buf, counts = ctx.call_cells(d, n, expected_cells=100)
        ctx.synchronize()
        assert counts == ia.CellCounts(**tot) and buf.download(np.uint8, n).tobytes() == cls.tobytes()
        buf.free()
        assert ctx.call_cells(d, n, top=7, by_reads=True, d_class=False) == (None, ia.CellCounts(**want[1]))
        assert ctx.call_cells(d, n, min_umis=50, d_class=False)[1] == ia.CellCounts(**cnp.call_cells(recs, cnp.MIN, 50, False, table)[1])
        assert ctx.call_cells(d, n, min_umis=50, d_class=False, counts=False) == (None, None)
        with pytest.raises(ValueError):
            ctx.call_cells(d, n, min_umis=1, top=1)
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        other.close()
        ar.free()


def _cell_records(recs, mode, param):
    """(the sorted records, those of them that belong to cells, the totals)."""
    s = count_np.sort_records(recs)
    cls, tot = cnp.call_cells(s, mode, param)
    return s, s[cls == cnp.CELL], tot


@pytest.mark.parametrize("n", [2561, 100_003])
@pytest.mark.parametrize("mode,param", [(cnp.MIN, 3), (cnp.TOP, 20), (cnp.ORDMAG, 30)])
def test_sort_call_select_barcode_counts(ia, ctx, n, mode, param):
    rng = np.random.default_rng(0x31600 + n)
    recs = _shape("knee", n, 0)[0][rng.permutation(n)]
    _, cells, tot = _cell_records(recs, mode, param)
    assert 0 < tot["cells"] < tot["barcodes"]
    d, tmp, d_class = ctx.upload(recs), ctx.alloc(24 * n), ctx.alloc(n)
    ctx.sort_records(d, tmp, n)
    kw = {cnp.MIN: "min_umis", cnp.TOP: "top", cnp.ORDMAG: "expected_cells"}[mode]
    _, counts = ctx.call_cells(d, n, d_class=d_class, **{kw: param})
    assert counts == ia.CellCounts(**tot)
    out, k = ctx.select_records(d, d_class, n, 1 << ia.CELL)
    assert k == tot["reads_cells"]
    ctx.synchronize()
    assert out.download(cnp.REC, k).tobytes() == cells.tobytes(), "exactly the records of the cells, still sorted"
    b, c, u = ctx.barcode_counts(out, k)
    _, reads, umis = cnp.barcode_table(cells)
    assert len(b) == tot["cells"] and c.tolist() == reads.tolist() and u.tolist() == umis.tolist()
    assert b.tolist() == cells["barcode"][cnp.barcode_table(cells)[0]].tolist()
    for x in (d, tmp, d_class, out):
        x.free()


def test_count_file_cells(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len = 16
    rng = np.random.default_rng(0x31700)
    recs = cnp.knee(rng, 30, 500, cell_umis=(50, 100), reads_per_umi=2)
    recs["index"] = recs["umi"] % np.uint64(3)
    recs = recs[rng.permutation(len(recs))]
    n = len(recs)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    text = lambda c: "".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(bc_len))
    _, cells, tot = _cell_records(recs, cnp.ORDMAG, 30)
    assert tot["cells"] == 30
    b, i, reads, umis = count_np.brute_force_matrix(cells)
    r = subprocess.run([str(exe), "--cells=expected:30", str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    matrix = [l for l in r.stdout.splitlines() if not l.startswith("#")]
    assert matrix == [f"{text(bb)}\t{ii}\t{uu}\t{rr}" for bb, ii, rr, uu in zip(b.tolist(), i.tolist(), reads.tolist(), umis.tolist())]
    assert (f"{n} records: barcodes {tot['barcodes']}, cells {tot['cells']}, threshold {tot['threshold']}, baseline {tot['baseline']}; "
            f"reads of cells {tot['reads_cells']}, of background {tot['reads_background']}; "
            f"umis of cells {tot['umis_cells']}, of background {tot['umis_background']}") in r.stderr
