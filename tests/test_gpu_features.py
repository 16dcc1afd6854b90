"""Per-feature metrics and the feature filter on the device (ibu_feature_metrics, ibu_filter_features): every comparison is byte for
byte against the numpy statement of the semantics in tests/feature_np.py, the totals included; every call goes through the C ABI,
and every buffer — the columns at exactly 8 B per feature, d_class at exactly n bytes, d_verdict at exactly n_features bytes — is
carved at its contract size out of the guard-zone arena of tests/test_gpu_count.py.  The records are compared after every case: they
are never written."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import count_np
from tests import feature_np as fnp
from tests.test_gpu_count import PATTERN, _arena, _p

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 127, 128, 129, 255, 2559, 2561, 100_003]
SEG, TILE = 8192, 128                                            # runs_walk.hpp: records per segment / per tile
SEAMS = [TILE * 3, TILE * 63, TILE * 65, SEG, 2 * SEG, 12 * SEG]
NS = SIZES + [s + d for s in SEAMS for d in (-1, 0, 1)]
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
NFS = [1, 64, 65, 70_000]
SHAPES = ["one_feature", "own_feature", "neighbours", "seam", "span", "out_of_range", "random"]
BIG = 1_000_003
GRID = [(n, skew, shape) for n, skew, shape in itertools.product(NS, SKEWS, SHAPES) if shape != "span" or n > 4 * SEG + 16]
GRID += [(BIG, 0, "own_feature"), (BIG, 8, "random")]            # one size of 1e6, for two shapes only
assert len(set(NS)) == len(NS) == 29 and len(GRID) == 2 * (29 * 6 + 4) + 2, len(GRID)
# one test per (size, base skew), its shapes inside it: the suite counts its tests in thousands already, and a case here is milliseconds
GROUPS = {}
for _n, _skew, _shape_name in GRID:
    GROUPS.setdefault((_n, _skew), []).append(_shape_name)
assert len(GROUPS) == 2 * 29 + 2
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


def _metrics(ia, ctx, d, n, word, nf, flags, cols, want_totals=True, stream=None):
    """One ibu_feature_metrics call through the C ABI -> the four totals (None without them); cols = three DeviceBuffers or None."""
    t = (C.c_uint64 * 4)(*[GARBAGE] * 4) if want_totals else None
    ia._check(ia.lib.ibu_feature_metrics(ctx._c, _p(d), n, word, nf, flags, *[_p(c) for c in cols], t, stream))
    return tuple(int(x) for x in t) if want_totals else None


def _garbage_counts():
    from ibu_amd import _lib
    return _lib.CFeatureFilterCounts((C.c_uint64 * 3)(*[GARBAGE] * 3), (C.c_uint64 * 4)(*[GARBAGE] * 4), GARBAGE)


def _filter(ia, ctx, d, n, word, nf, cols, lim, d_class, d_verdict, want_counts=True, stream=None):
    """One ibu_filter_features call through the C ABI -> the totals as feature_np states them (None without counts)."""
    from ibu_amd import _lib
    c = _garbage_counts()
    l = _lib.CFeatureLimits(*[lim[f] for f in fnp.LIMITS])
    ia._check(ia.lib.ibu_filter_features(ctx._c, _p(d), n, word, nf, *[_p(x) for x in cols], C.byref(l), _p(d_class), _p(d_verdict),
                                         C.byref(c) if want_counts else None, stream))
    if not want_counts:
        return None
    return {"features_by_class": tuple(int(x) for x in c.features_by_class), "reads_by_class": tuple(int(x) for x in c.reads_by_class),
            "reserved": int(c.reserved)}


def _palette(nf):
    """The values the second and third words take: the ends and the middle of the table, the two values just past it, and three of
    2^32 and more whose low bits name a valid feature."""
    return np.array([0, nf // 2, nf - 1, nf, nf + 1, 1 << 32, (1 << 32) + nf - 1, (1 << 32) + nf // 2], np.uint64)


def _valid(nf):
    return np.array([0, nf // 2, nf - 1, nf // 3, (2 * nf) // 3, nf // 5], np.uint64)


def _base(n, nf):
    """Barcodes of three records: two or three pairs, three triples; a quarter of the features out of range."""
    r = np.zeros(n, fnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.int64)
    pal = np.concatenate([_valid(nf), _palette(nf)[[3, 6]]])
    w[:, 0] = (i // 3).astype(np.uint64)
    w[:, 1] = pal[(i // 3 + (i % 3) // 2) % 8]
    w[:, 2] = pal[i % 8]
    return r, w


def _seam(n, nf, head, d, straddle):
    """Around every seam row s + d + head that fits.  straddle False: a pair of ten records (five triples) ends just in front of the
    row and another of ten begins on it, in the same barcode at every other seam.  straddle True: one pair of ten records lies across
    the row, and so does the second of its three triples."""
    r, w = _base(n, nf)
    laid = []
    for k, s in enumerate(SEAMS):
        row = s + d + head
        big = (1 << 40) + 2 * k
        fa, fb = np.uint64((7 * k) % nf), np.uint64((7 * k + 1) % nf if k & 1 else (7 * k) % nf)
        if straddle:
            if row - 5 < 0 or row + 5 > n:
                continue
            w[row - 5:row + 5, 0], w[row - 5:row + 5, 1], w[row - 5:row + 5, 2] = big, fa, [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
        else:
            if row - 10 < 0 or row + 10 > n:
                continue
            w[row - 10:row, 0], w[row - 10:row, 1], w[row - 10:row, 2] = big, fa, np.repeat(np.arange(5, dtype=np.uint64), 2)
            # the same feature in the next barcode (even k): the head on the seam row leaves w1 unchanged; another feature, same barcode (odd k)
            w[row:row + 10, 0], w[row:row + 10, 1], w[row:row + 10, 2] = big + (0 if k & 1 else 1), fb, np.repeat(np.arange(5, dtype=np.uint64), 2)
        laid.append(row)
    return r, laid


def _shape(shape, n, nf, skew, d=0, straddle=False):
    head = min(skew // 8, n)
    i = np.arange(n, dtype=np.int64)
    if shape in ("seam", "span"):
        if shape == "seam":
            return _seam(n, nf, head, d, straddle)[0]
        r, w = _base(n, nf)                                      # one pair from in front of the second segment to behind the fourth
        a, b = head + SEG - 6, head + 4 * SEG + 9
        w[a:b, 0], w[a:b, 1], w[a:b, 2] = 1 << 41, nf - 1, ((np.arange(b - a) // 7) % 5).astype(np.uint64)
        return r
    r = np.zeros(n, fnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    if shape == "one_feature":                                   # every atomic lands on one counter
        w[:, 0], w[:, 1], w[:, 2] = (i // 5).astype(np.uint64), nf - 1, (nf - 1) * ((i // 2) % 2)
    elif shape == "own_feature":                                 # every pair (of 1 .. 3 records) has its own feature
        pair = (i * 2 + 1) // 5
        w[:, 0], w[:, 1], w[:, 2] = (pair // 3).astype(np.uint64), (pair % nf).astype(np.uint64), (i % nf).astype(np.uint64)
    elif shape == "neighbours":                                  # barcodes of three records, four in a row with the same feature
        w[:, 0], w[:, 1], w[:, 2] = (i // 3).astype(np.uint64), ((i // 12) % nf).astype(np.uint64), _valid(nf)[(i // 2) % 6]
    elif shape == "out_of_range":
        pal = _palette(nf)
        w[:, 0], w[:, 1], w[:, 2] = (i // 7).astype(np.uint64), pal[(i // 2) % 8], pal[(i // 3) % 8]
    else:                                                        # an unstructured mix, sorted
        rng = np.random.default_rng(0x51300 + n + nf)
        pal = np.concatenate([_valid(nf), _palette(nf)])
        w[:, 0] = rng.integers(0, n // 20 + 2, n).astype(np.uint64)
        w[:, 1], w[:, 2] = pal[rng.integers(0, len(pal), n)], pal[rng.integers(0, len(pal), n) // 3]
        r = r[np.lexsort((w[:, 2], w[:, 1], w[:, 0]))]
    return r


def _limit_sets(table, word):
    """The limits a case is filtered with: none, the usual minimum on cells (umis for feature_word 2), and a mix from the table's
    own quantiles that reaches LOW and HIGH."""
    q = lambda c, f: int(np.sort(c)[int(f * (len(c) - 1))])
    reads, umis, cells = table
    out = [fnp.limits(), fnp.limits(min_cells=2) if word == 1 else fnp.limits(min_umis=2),
           fnp.limits(min_reads=max(q(reads, 0.3), 1), max_umis=max(q(umis, 0.9), 1), max_reads=max(q(reads, 0.95), 1))]
    if word == 1:
        out[2]["max_cells"] = max(q(cells, 0.8), 1)
    return out


def _same(buf, want, what):
    have = buf.download(want.dtype, len(want)) if len(want) else np.empty(0, want.dtype)
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {int(bad[0])}: {int(have[bad[0]])} for {int(want[bad[0]])}"


class _Buffers:
    """One arena for all the cases of a test (an allocation per case costs more than the case): the records at `skew`, two class
    arrays of exactly n bytes, and for every table size three columns of exactly 8 nf bytes and a verdict table of exactly nf."""

    def __init__(self, ia, ctx, n, skew, nfs):
        self.ar = _arena(ia, ctx, 24 * n, n, n, *[s for nf in nfs for s in (8 * nf, 8 * nf, 8 * nf, nf)])
        self.d = self.ar.carve(24 * n, skew)
        self.d_classes = [self.ar.carve(n, 0), self.ar.carve(n, 3)]   # (with the one record a skewed base peels: 16-bit and byte stores)
        self.tables = {nf: ([self.ar.carve(8 * nf, 8 * (j & 1)) for j in range(3)], self.ar.carve(nf, 1)) for nf in nfs}


def _check_case(ia, ctx, bufs, recs, n, nf):
    """Both feature words: the three columns and the totals, then the filter under several limits into d_class at exactly n bytes
    and d_verdict at exactly nf bytes."""
    d, d_classes, (cols, d_verdict) = bufs.d, bufs.d_classes, bufs.tables[nf]
    if n:
        d.upload(recs)
    reached = set()
    for word in (1, 2):
        what = f"n_features {nf}, word {word}"
        table, totals = fnp.feature_metrics(recs, nf, word)
        given = cols if word == 1 else cols[:2] + [None]
        assert _metrics(ia, ctx, d, n, word, nf, 0, given) == totals, what
        ctx.synchronize()
        for name, col, want in zip(fnp.COLUMNS, given, table):
            if col is not None:
                _same(col, want, f"{what}: {name}")
        features = fnp.record_features(recs, nf, word)
        for i, lim in enumerate(_limit_sets(table if word == 1 else (table[0], table[1], table[1]), word)):
            d_class = d_classes[(i + word) & 1]
            v, cls, tot = fnp.filter_features(recs, nf, word, table, lim, features)
            assert _filter(ia, ctx, d, n, word, nf, given, lim, d_class, d_verdict) == tot, (what, lim)
            _same(d_verdict, v, f"{what} {lim}: verdicts")
            _same(d_class, cls, f"{what} {lim}: class bytes")
            reached |= {c for c in range(3) if tot["features_by_class"][c]} | {c for c in range(4) if tot["reads_by_class"][c]}
    assert n == 0 or d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
    return reached


@pytest.mark.parametrize("n,skew", list(GROUPS))
def test_metrics_and_filter_match_numpy(ia, ctx, n, skew):
    nfs = NFS if n < BIG else NFS[2:]
    bufs = _Buffers(ia, ctx, n, skew, nfs)
    try:
        for shape, nf in itertools.product(GROUPS[n, skew], nfs):
            variants = [(d, s) for d in (-1, 0, 1) for s in (False, True)] if shape == "seam" and n > TILE * 3 else [(0, False)]
            reached = set()
            try:
                for d, straddle in variants:
                    reached |= _check_case(ia, ctx, bufs, _shape(shape, n, nf, skew, d, straddle), n, nf)
                bufs.ar.check(f"n_features {nf}")
            except AssertionError as e:
                raise AssertionError(f"shape {shape}: {e}") from e
            if shape in ("out_of_range", "random") and n >= 2559 and nf > 1:
                assert reached == {0, 1, 2, 3}, (shape, nf, reached)
    finally:
        bufs.ar.free()


def test_the_shapes_have_what_they_claim():
    n, nf = 100_003, 65
    for d, straddle in itertools.product((-1, 0, 1), (False, True)):
        recs, laid = _seam(n, nf, 1, d, straddle)
        assert laid == [s + d + 1 for s in SEAMS], (d, laid)
        w = recs.view(np.uint64).reshape(-1, 3)
        for k, row in enumerate(laid):
            if straddle:
                assert (w[row - 1] == w[row]).all() and w[row - 6, 0] != w[row - 5, 0] and w[row + 5, 0] != w[row + 4, 0], "one triple lies across the row"
            else:
                assert (w[row - 10:row, :2] == w[row - 1, :2]).all() and (w[row:row + 10, :2] == w[row, :2]).all()
                assert (w[row - 1, 0] != w[row, 0]) == (k % 2 == 0) and (w[row - 1, 1] == w[row, 1]) == (k % 2 == 0), "a barcode head that leaves w1 unchanged"
    recs = _shape("span", n, nf, 8)
    (reads, umis, cells), _ = fnp.feature_metrics(recs, nf, 1)
    w = recs.view(np.uint64).reshape(-1, 3)
    long = np.flatnonzero(w[:, 0] == 1 << 41)
    assert long[0] < 1 + SEG and long[-1] > 1 + 4 * SEG and len(long) == 3 * SEG + 15, "three whole segments"
    recs = _shape("neighbours", n, nf, 0)
    (reads, umis, cells), _ = fnp.feature_metrics(recs, nf, 1)
    pairs = count_np.pair_counts(recs)
    assert len(pairs[0]) == (n + 2) // 3 == int(cells.sum()) and len(np.unique(pairs[1])) * 4 < len(pairs[0]), "every barcode is a cell of its feature"
    recs = _shape("one_feature", n, nf, 0)
    assert fnp.feature_metrics(recs, nf, 1)[0][0].tolist() == [0] * 64 + [n]
    recs = _shape("out_of_range", n, nf, 0)
    values = set(np.unique(recs["umi"]).tolist())
    assert {nf, nf + 1, 1 << 32, (1 << 32) + nf - 1} <= values and fnp.feature_metrics(recs, nf, 1)[1][3] > n // 2


def test_forms_of_the_metrics_call(ia, ctx):
    n, nf = 100_003, 65
    recs = _shape("random", n, nf, 0)
    (reads, umis, cells), totals = fnp.feature_metrics(recs, nf, 1)
    table2, totals2 = fnp.feature_metrics(recs, nf, 2)
    pattern = np.full(8 * nf, PATTERN, np.uint8).tobytes()
    ar = _arena(ia, ctx, 24 * n, *[8 * nf] * 3)
    other = ia.Context(0)
    try:
        d = ar.carve(24 * n, 8)
        cols = [ar.carve(8 * nf, 8 * (j & 1)) for j in range(3)]
        d.upload(recs)
        wrap = lambda buf, off: ia.DeviceBuffer.wrap(ctx, buf.ptr + off, 8)
        # every invalid argument is refused before anything is touched, the totals included
        bad = [(d, n, 0, nf, 0, cols), (d, n, 3, nf, 0, cols), (d, n, 1, 0, 0, cols), (d, n, 1, (1 << 32) + 1, 0, cols), (d, n, 1, nf, 2, cols),
               (d, n, 1, nf, 0, [wrap(cols[0], 4)] + cols[1:]), (d, n, 1, nf, 0, cols[:2] + [wrap(cols[2], 4)]), (d, n, 2, nf, 0, cols),
               (None, 1, 1, nf, 0, cols), (wrap(d, 4), 1, 1, nf, 0, cols), (d, 1 << 40, 1, nf, 0, cols)]
        for k, (buf, count, word, f, flags, given) in enumerate(bad):
            t = (C.c_uint64 * 4)(*[GARBAGE] * 4)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_feature_metrics(ctx._c, _p(buf), count, word, f, flags, *[_p(c) for c in given], t, None))
            assert ei.value.kind == "InvalidArg" and list(t) == [GARBAGE] * 4, k
        ar.check("refused calls")
        assert all(c.download(np.uint8, 8 * nf).tobytes() == pattern for c in cols), "a refused call writes nothing"
        # every subset of NULL columns, with the totals and without
        for mask in range(8):
            for c in cols:
                c.upload(np.full(8 * nf, PATTERN, np.uint8))
            given = [c if mask >> j & 1 else None for j, c in enumerate(cols)]
            got = _metrics(ia, ctx, d, n, 1, nf, 0, given, want_totals=bool(mask & 1) or mask == 0)
            assert got in (totals, None), mask
            ctx.synchronize()
            for j, (c, want) in enumerate(zip(cols, (reads, umis, cells))):
                assert c.download(np.uint8, 8 * nf).tobytes() == (want.tobytes() if mask >> j & 1 else pattern), (mask, j)
        ar.check("subsets of the columns")
        # two runs give the same columns; a stream of another context; feature_word 2 leaves d_cells alone
        first = [c.download(np.uint64, nf).tobytes() for c in cols]
        assert _metrics(ia, ctx, d, n, 1, nf, 0, cols, stream=other.stream) == totals
        other.synchronize(other.stream)
        assert [c.download(np.uint64, nf).tobytes() for c in cols] == first == [reads.tobytes(), umis.tobytes(), cells.tobytes()]
        assert _metrics(ia, ctx, d, n, 2, nf, 0, cols[:2] + [None]) == totals2
        ctx.synchronize()
        assert [c.download(np.uint64, nf).tobytes() for c in cols] == [table2[0].tobytes(), table2[1].tobytes(), cells.tobytes()]
        # accumulating over two halves cut where a barcode begins is one call ...
        cut = int(np.flatnonzero(recs["barcode"][1:] != recs["barcode"][:-1])[n // 40]) + 1
        halves = lambda k: (ia.DeviceBuffer.wrap(ctx, d.ptr, 24 * k), k, ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * k, 24 * (n - k)), n - k)
        a, na, b, nb = halves(cut)
        t1 = _metrics(ia, ctx, a, na, 1, nf, 0, cols)
        t2 = _metrics(ia, ctx, b, nb, 1, nf, ia.FEATURE_ACCUMULATE, cols)
        ctx.synchronize()
        assert tuple(x + y for x, y in zip(t1, t2)) == totals and t2 == fnp.feature_metrics(recs[cut:], nf, 1)[1], "the totals are those of one call"
        assert [c.download(np.uint64, nf).tobytes() for c in cols] == first
        # ... and cut inside a pair (and a triple) it gives the documented extra cell (and UMI)
        w = recs.view(np.uint64).reshape(-1, 3)
        inside = int(np.flatnonzero((w[1:] == w[:-1]).all(axis=1) & (w[1:, 1] < nf))[n // 50]) + 1
        a, na, b, nb = halves(inside)
        _metrics(ia, ctx, a, na, 1, nf, 0, cols, want_totals=False)
        _metrics(ia, ctx, b, nb, 1, nf, ia.FEATURE_ACCUMULATE, cols, want_totals=False)
        ctx.synchronize()
        extra = np.zeros(nf, np.uint64)
        extra[int(w[inside, 1])] = 1
        want = fnp.feature_metrics(recs[inside:], nf, 1, into=fnp.feature_metrics(recs[:inside], nf, 1)[0])[0]
        assert [x.tobytes() for x in want] == [reads.tobytes(), (umis + extra).tobytes(), (cells + extra).tobytes()]
        assert [c.download(np.uint64, nf).tobytes() for c in cols] == [x.tobytes() for x in want]
        # n == 0: the columns are zeroed unless accumulating, and the totals are 0
        assert _metrics(ia, ctx, None, 0, 1, nf, ia.FEATURE_ACCUMULATE, cols) == (0, 0, 0, 0)
        assert [c.download(np.uint64, nf).tobytes() for c in cols] == [x.tobytes() for x in want]
        assert _metrics(ia, ctx, None, 0, 1, nf, 0, cols) == (0, 0, 0, 0)
        assert all(c.download(np.uint8, 8 * nf).tobytes() == bytes(8 * nf) for c in cols)
        ar.check("forms of the metrics call")
        # the Python wrapper
        t = ctx.feature_metrics(d, n, nf)
        assert isinstance(t, ia.FeatureTable) and t.totals == totals and t.n_features == nf
        assert [c.download(np.uint64, nf).tobytes() for c in t[:3]] == first
        t = ctx.feature_metrics(a, na, nf, totals=False)
        t = ctx.feature_metrics(b, nb, nf, accumulate_into=t)
        assert [c.download(np.uint64, nf).tobytes() for c in t[:3]] == [x.tobytes() for x in want]
        t2 = ctx.feature_metrics(d, n, nf, feature_word=2)
        assert t2.cells is None and t2.totals == totals2 and t2.umis.download(np.uint64, nf).tobytes() == table2[1].tobytes()
        for x in (*t[:3], *t2[:2]):
            x.free()
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        other.close()
        ar.free()


def test_forms_of_the_filter_call(ia, ctx):
    n, nf = 100_003, 65
    recs = _shape("random", n, nf, 0)
    other_recs = _shape("neighbours", 2561, nf, 0)               # "the called cells": the columns come from these
    table, _ = fnp.feature_metrics(other_recs, nf, 1)
    ar = _arena(ia, ctx, 24 * n, 24 * 2561, n + 8, *[8 * nf] * 3, nf)
    other = ia.Context(0)
    try:
        d, d_other = ar.carve(24 * n, 8), ar.carve(24 * 2561, 0)
        d_class_all, d_verdict = ar.carve(n + 8, 0), ar.carve(nf, 3)
        cols = [ar.carve(8 * nf, 8 * (j & 1)) for j in range(3)]
        d.upload(recs)
        d_other.upload(other_recs)
        wrap = lambda buf, off, size=8: ia.DeviceBuffer.wrap(ctx, buf.ptr + off, size)
        _metrics(ia, ctx, d_other, 2561, 1, nf, 0, cols, want_totals=False)
        ctx.synchronize()
        q = lambda c, f: int(np.sort(c)[int(f * (len(c) - 1))])
        # every limit alone, then combined; the columns of records A applied to records B; d_class at every offset of a 16-byte word
        names = [("min_reads", 0, 0.9), ("max_reads", 0, 0.5), ("min_umis", 1, 0.9), ("max_umis", 1, 0.5), ("min_cells", 2, 0.9), ("max_cells", 2, 0.5)]
        lims = [fnp.limits(**{name: max(q(table[j], f), 1)}) for name, j, f in names]
        lims.append(fnp.limits(min_reads=max(q(table[0], 0.2), 1), max_reads=max(q(table[0], 0.9), 1), min_umis=1, max_umis=max(q(table[1], 0.8), 1),
                               min_cells=2, max_cells=max(q(table[2], 0.7), 2)))
        seen = set()
        for k, lim in enumerate(lims):
            d_class = wrap(d_class_all, k, n)
            v, cls, tot = fnp.filter_features(recs, nf, 1, table, lim)
            assert _filter(ia, ctx, d, n, 1, nf, cols, lim, d_class, d_verdict) == tot, lim
            _same(d_verdict, v, f"{lim}: verdicts")
            _same(d_class, cls, f"{lim}: classes at offset {k}")
            seen |= set(v.tolist())
            d_class_all.upload(np.full(n + 8, PATTERN, np.uint8))
        assert seen == {0, 1, 2}
        # zeroed limits pass everything except the unknown features; a column whose limits are 0 may be NULL
        v, cls, tot = fnp.filter_features(recs, nf, 1, table, fnp.limits())
        assert not v.any() and set(cls.tolist()) == {0, 3}
        for given in (cols, [None] * 3, [cols[0], None, None]):
            assert _filter(ia, ctx, d, n, 1, nf, given, fnp.limits(), wrap(d_class_all, 0, n), d_verdict) == tot
            _same(wrap(d_class_all, 0, n), cls, "zeroed limits")
        lim = lims[-1]
        v, cls, tot = fnp.filter_features(recs, nf, 1, table, lim)
        # d_class NULL: totals only; d_verdict NULL: the table lives in the context; neither totals nor classes: the verdicts alone
        d_class_all.upload(np.full(n + 8, PATTERN, np.uint8))
        assert _filter(ia, ctx, d, n, 1, nf, cols, lim, None, d_verdict) == tot
        assert _filter(ia, ctx, d, n, 1, nf, cols, lim, None, None) == tot
        assert d_class_all.download(np.uint8, n + 8).tobytes() == bytes([PATTERN]) * (n + 8)
        assert _filter(ia, ctx, d, n, 1, nf, cols, lim, wrap(d_class_all, 1, n), None, want_counts=False) is None
        ctx.synchronize()
        _same(wrap(d_class_all, 1, n), cls, "classes only, the verdict table in the context")
        d_verdict.upload(np.full(nf, PATTERN, np.uint8))
        assert _filter(ia, ctx, d, n, 1, nf, cols, lim, None, d_verdict, want_counts=False) is None
        ctx.synchronize()
        _same(d_verdict, v, "verdicts alone")
        # n == 0 still fills the verdicts and features_by_class, and touches no record
        d_verdict.upload(np.full(nf, PATTERN, np.uint8))
        assert _filter(ia, ctx, None, 0, 1, nf, cols, lim, None, d_verdict) == dict(tot, reads_by_class=(0, 0, 0, 0))
        _same(d_verdict, v, "n == 0")
        # feature_word 2 on a stream of another context, with the columns of the same records
        table2, _ = fnp.feature_metrics(recs, nf, 2)
        _metrics(ia, ctx, d, n, 2, nf, 0, cols[:2] + [None], want_totals=False)
        ctx.synchronize()
        lim2 = fnp.limits(min_umis=max(q(table2[1], 0.5), 1), max_reads=max(q(table2[0], 0.9), 1))
        v2, cls2, tot2 = fnp.filter_features(recs, nf, 2, table2, lim2)
        assert _filter(ia, ctx, d, n, 2, nf, cols[:2] + [None], lim2, wrap(d_class_all, 3, n), d_verdict, stream=other.stream) == tot2
        other.synchronize(other.stream)
        _same(wrap(d_class_all, 3, n), cls2, "feature_word 2")
        _same(d_verdict, v2, "feature_word 2: verdicts")
        ar.check("forms of the filter call")
        # every invalid argument is refused before anything is touched, `counts` included
        from ibu_amd import _lib
        d_class_all.upload(np.full(n + 8, PATTERN, np.uint8))
        d_verdict.upload(np.full(nf, PATTERN, np.uint8))
        bad = [(d, n, 0, nf, cols, lim), (d, n, 3, nf, cols, lim), (d, n, 1, 0, cols, lim), (d, n, 1, (1 << 32) + 1, cols, lim), (d, n, 1, nf, cols, None),
               (d, n, 1, nf, [wrap(cols[0], 4)] + cols[1:], lim), (d, n, 1, nf, [None] + cols[1:], lim), (d, n, 1, nf, cols[:2] + [None], lim),
               (d, n, 1, nf, [cols[0], None, cols[2]], fnp.limits(max_umis=5)), (None, 1, 1, nf, cols, lim), (wrap(d, 4), 1, 1, nf, cols, lim),
               (d, 1 << 40, 1, nf, cols, lim)]
        for k, (buf, count, word, f, given, l) in enumerate(bad):
            c = _garbage_counts()
            cl = _lib.CFeatureLimits(*[l[x] for x in fnp.LIMITS]) if l else None
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_filter_features(ctx._c, _p(buf), count, word, f, *[_p(x) for x in given], C.byref(cl) if cl else None,
                                                     _p(d_class_all), _p(d_verdict), C.byref(c), None))
            assert ei.value.kind == "InvalidArg" and [*c.features_by_class, *c.reads_by_class, c.reserved] == [GARBAGE] * 8, k
        ar.check("refused calls")
        assert d_class_all.download(np.uint8, n + 8).tobytes() == bytes([PATTERN]) * (n + 8) and d_verdict.download(np.uint8, nf).tobytes() == bytes([PATTERN]) * nf
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        other.close()
        ar.free()


def test_count_file_features(ia, tmp_path):
    """examples/count_file.cpp --features --n-features --feature-table end to end: the table of every feature, and the matrix of the
    features that pass, counted without a second sort."""
    import os
    import subprocess
    from ibu_amd import _lib
    from tests import cells_np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len, nf = 16, 40
    rng = np.random.default_rng(0x51700)
    recs = cells_np.knee(rng, 30, 200, cell_umis=(50, 100), reads_per_umi=2)
    recs["index"] = (recs["umi"] * np.uint64(7) + recs["barcode"]) % (np.uint64(20) + recs["barcode"] % np.uint64(25))   # 20 .. 44 features: some are unknown
    recs = recs[rng.permutation(len(recs))]
    n = len(recs)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    swapped = count_np.sort_records(count_np.swap(recs))
    table, totals = fnp.feature_metrics(swapped, nf, 1)
    min_cells, min_umis = int(np.sort(table[2])[nf // 2]), int(np.sort(table[1])[nf // 4])
    v, cls, tot = fnp.filter_features(swapped, nf, 1, table, fnp.limits(min_cells=min_cells, min_umis=min_umis))
    assert 0 < tot["features_by_class"][0] < nf and tot["reads_by_class"][3] == totals[3] > 0, tot
    b, i, reads, umis = count_np.brute_force_matrix(count_np.swap(swapped[cls == fnp.PASS]))
    text = lambda c: "".join("ACGT"[(int(c) >> (2 * k)) & 3] for k in range(bc_len))
    r = subprocess.run([str(exe), f"--features=mincells:{min_cells},minumi:{min_umis}", f"--n-features={nf}", f"--feature-table={tmp_path / 'table.txt'}",
                        str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    matrix = [l for l in r.stdout.splitlines() if not l.startswith("#")]
    assert matrix == [f"{text(bb)}\t{ii}\t{uu}\t{rr}" for bb, ii, rr, uu in zip(b.tolist(), i.tolist(), reads.tolist(), umis.tolist())]
    assert f"{n} records: {nf} features: reads {totals[0]}, umis {totals[1]}, cells {totals[2]}; reads of other index values {totals[3]}" in r.stderr
    fc, rc = tot["features_by_class"], tot["reads_by_class"]
    assert f"{n} records: features pass {fc[0]}, low {fc[1]}, high {fc[2]}; reads pass {rc[0]}, low {rc[1]}, high {rc[2]}, unknown {rc[3]}" in r.stderr
    want = [f"{k}\t{int(table[0][k])}\t{int(table[1][k])}\t{int(table[2][k])}" for k in range(nf) if table[0][k]]
    assert (tmp_path / "table.txt").read_text().splitlines() == want


@pytest.mark.parametrize("n", [2561, 100_003])
def test_pipeline_filtered_matrix_without_a_second_sort(ia, ctx, n):
    """count_matrix(leave_swapped=True) -> feature_metrics -> filter_features -> select_records -> pair_counts is the numpy matrix
    restricted to the kept features."""
    nf = 40
    rng = np.random.default_rng(0x51600 + n)
    recs = count_np.make_records(rng, n, 16, max(n // 60, 3), 48, 12, high_bit=False)   # index values 0 .. 47: eight are unknown features
    d, tmp = ctx.upload(recs), ctx.alloc(24 * n)
    matrix = ctx.count_matrix(d, tmp, n, leave_swapped=True)
    (b, i, reads, umis), swapped = count_np.count_matrix(recs)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(matrix, (b, i, reads, umis)))
    table = ctx.feature_metrics(d, n, nf)
    (want_reads, want_umis, want_cells), totals = fnp.feature_metrics(swapped, nf, 1)
    assert table.totals == totals and totals[3] > 0
    assert [c.download(np.uint64, nf).tobytes() for c in table[:3]] == [want_reads.tobytes(), want_umis.tobytes(), want_cells.tobytes()]
    # the columns are the column sums of the matrix
    ok = i < nf
    assert want_cells.tolist() == np.bincount(i[ok].astype(np.int64), minlength=nf).tolist()
    assert want_umis.tolist() == np.bincount(i[ok].astype(np.int64), weights=umis[ok].astype(np.float64), minlength=nf).astype(np.uint64).tolist()
    min_cells = int(np.sort(want_cells)[nf // 3]) + 1
    v, cls, tot = fnp.filter_features(swapped, nf, 1, (want_reads, want_umis, want_cells), fnp.limits(min_cells=min_cells))
    assert 0 < tot["features_by_class"][0] < nf and tot["reads_by_class"][3] == totals[3]
    d_verdict = ctx.alloc(nf)
    d_class, counts = ctx.filter_features(d, n, table, min_cells=min_cells, d_verdict=d_verdict)
    assert counts == ia.FeatureFilterCounts(tot["features_by_class"], tot["reads_by_class"])
    assert d_verdict.download(np.uint8, nf).tobytes() == v.tobytes() and d_class.download(np.uint8, n).tobytes() == cls.tobytes()
    out, k = ctx.select_records(d, d_class, n, 1 << ia.FEATURE_PASS)
    ctx.synchronize()
    assert k == tot["reads_by_class"][0] and out.download(fnp.REC, k).tobytes() == swapped[cls == fnp.PASS].tobytes(), "the kept features, still sorted"
    kept = (i < nf) & (v[np.minimum(i, nf - 1).astype(np.int64)] == fnp.PASS)
    got = ctx.pair_counts(out, k)
    assert all(g.tobytes() == w[kept].tobytes() for g, w in zip(got, (b, i, reads, umis))), "the matrix restricted to the kept features"
    assert ctx.filter_features(d, n, table, d_class=False)[1].features_by_class == (nf, 0, 0)
    assert ctx.filter_features(d, n, table, min_umis=1, d_class=False, counts=False) == (None, None)
    for x in (d, tmp, d_class, d_verdict, out, *table[:3]):
        x.free()
