"""The second level of the aggregations at its own seams.  The segment walk leaves per-block or per-segment summaries, and a small
kernel scans them — four per thread, 256 per wave, 1024 per round — so that a run across many blocks is settled once:
ibu_k_molecules_verdict / _chains / _fix over candidate blocks, ibu_k_saturation_stitch and ibu_k_runs_scan over segments.  The
per-feature files lay their structure at the walk's row seams; here it is laid at the thread, wave and round boundaries of those
scans, at the smallest sizes that have them (1024 blocks and more: 1.05 M candidates; 1024 segments and more: 8.4 M records).
Every comparison is exact against the numpy statements (tests/molecule_np.py, saturation_np.py, count_np.py, cells_np.py), every
call goes through the C ABI, every buffer is carved at its contract size out of an arena with guard zones, and the records are
compared after every case: they are never written."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cells_np
from tests import count_np as cnp
from tests import molecule_np as mnp
from tests import saturation_np as snp
from tests.test_gpu_cells import _call as _call_cells
from tests.test_gpu_count import PATTERN, _arena, _download, _p, _pair_counts, _same
from tests.test_gpu_molecules import _check_case as _check_molecules
from tests.test_gpu_molecules import _classify
from tests.test_gpu_saturation import _curve

pytestmark = pytest.mark.gpu

SEG, TILE = 8192, 128                                            # runs_walk.hpp: records per segment / per tile
MOL_BLOCK = 1024                                                 # k_molecules.hip: kMolBlock = kSortThreads * kMolItems candidates per verdict block
PER_THREAD = 4                                                   # summaries per thread: kMolItems (chains), the 4 of the stitch and of ibu_k_runs_scan
PER_WAVE = 256                                                   # ... per wave: 64 lanes x 4
PER_ROUND = 1024                                                 # ... per round of the one workgroup: kSortThreads x 4
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
SEAM_BLOCKS = (1, 2, 4, 255, 256, 257, 512, 768, 1023, 1024, 1025, 1028)
SEAM_SEGMENTS = (4, 8, 252, 256, 260, 512, 768, 1020, 1024, 1028)
BIG_N = 8_437_891                                                # 1030 segments of 8192 records and 131 more
assert (MOL_BLOCK, SEAM_BLOCKS, snp.SEG, cnp.SEG) == (mnp.MOL_BLOCK, mnp.SEAM_BLOCKS, SEG, SEG)
# a thread, a wave and the round boundary, with the summaries on either side of each, are among the seams of both scans
assert {PER_THREAD, PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, 2 * PER_WAVE, 3 * PER_WAVE, PER_ROUND - 1, PER_ROUND, PER_ROUND + 1, PER_ROUND + PER_THREAD} <= set(SEAM_BLOCKS)
assert {PER_THREAD, PER_WAVE - PER_THREAD, PER_WAVE, PER_WAVE + PER_THREAD, 2 * PER_WAVE, 3 * PER_WAVE, PER_ROUND - PER_THREAD, PER_ROUND, PER_ROUND + PER_THREAD} <= set(SEAM_SEGMENTS)
# the molecule sizes: one round; a second round of one block of one candidate; a second round of eight blocks, the last one partial
assert [-(-c // MOL_BLOCK) for c in mnp.BLOCK_SIZES] == [1024, 1025, 1032] and [c % MOL_BLOCK for c in mnp.BLOCK_SIZES] == [0, 1, 7]


def _plan(n, skew):
    """seg_plan of runs_walk.hpp for a base `skew` bytes behind a 16-byte boundary -> (peeled rows, segments of the plan)."""
    head = min(skew // 8, n)
    main = (n - head) // TILE * TILE
    return head, -(-main // SEG) + 2


# 8 437 891 = 1030 x 8192 + 131: the 131 are one more tile, which is a tiled segment of its own, and a rest of 3 (2 behind a peeled
# record); with segment 0 (the peeled front) the plan has 1033 segments at both skews, 1031 of them tiled
assert [_plan(BIG_N, s) for s in SKEWS] == [(0, 1033), (1, 1033)] and max(SEAM_SEGMENTS) + 1 < 1031 and BIG_N > (PER_ROUND + 6) * SEG


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


# ---- 1. molecules: candidate-block seams ----------------------------------------------------------------------------------------
seam_plan = functools.lru_cache(maxsize=None)(mnp.seam_plan)
MOL_CASES = [(c, a) for c in mnp.BLOCK_SIZES for a in range(len(seam_plan(c)))]


@pytest.mark.parametrize("ncand,array", MOL_CASES)
def test_candidate_block_seams(ia, ctx, ncand, array):
    laid = seam_plan(ncand)[array]
    reads, mol_head, pieces = mnp.seam_table(ncand, laid)
    recs = mnp.lay_candidates(reads, mol_head)
    want = {f: mnp.classify(recs, f) for f in (False, True)}
    assert want[False][1]["candidates"] == ncand
    mnp.check_seam_table(reads, mol_head, pieces, recs, want)   # from the numpy side, before the device is asked
    for skew in SKEWS:
        try:
            _check_molecules(ia, ctx, recs, want, len(recs), skew)   # both tie modes, class bytes at offsets 0 and 3, the seven totals
        except AssertionError as e:
            raise AssertionError(f"{ncand} candidates, skew {skew}, laid {laid}: {e}") from e


def test_every_seam_block_is_laid_at_the_largest_size():
    big = mnp.BLOCK_SIZES[-1]
    laid = [x for a in seam_plan(big) for x in a]
    assert len(laid) == len(set(laid))
    for i, K in enumerate(SEAM_BLOCKS):
        mine = [s for k, s in laid if k == K]
        assert sorted(mine) == sorted(s for s in mnp.seam_specs(i) if s[0] != "span" or K >= 2), K   # (a span begins two blocks in front of K)
        names = {s[0] if s[0] != "head_last" else s[:2] for s in mine}
        assert names >= {"ends_on_seam", "head_second"} | {("head_last", d) for d in mnp.HEAD_LAST_D}, K
        assert ("span" in names) == (K >= 2), K
        for s in mine:                                           # the boundary candidate itself is what each piece is about
            p = mnp.seam_piece(s, K, big)
            assert p["lo"] < MOL_BLOCK * K < p["hi"] + 1 and any(c in (MOL_BLOCK * K - 1, MOL_BLOCK * K) for c, _ in p["head_checks"]), (K, s)
    spans = {s[1] for _, s in laid if s[0] == "span"}
    assert spans == set(mnp.WIN7) and {s[2] for _, s in laid if s[0] == "head_last" and s[1] >= 1024} == set(mnp.WIN5)
    assert all((K, ("span", "tie_seam")) in laid for K in (PER_WAVE, PER_ROUND)), "a tie across the wave seam and across the round seam"
    assert [s[1] for k, s in laid if s[0] == "long"] == list(mnp.LONG_VARIANTS)
    assert mnp.LONG[0] < PER_WAVE and mnp.LONG[1] > PER_ROUND, "the long molecule crosses every wave seam and the round seam"
    # the smaller sizes: everything up to the last block, which ends the data
    for c, top in zip(mnp.BLOCK_SIZES[:2], (1023, 1024)):
        ks = {k for a in seam_plan(c) for k, _ in a}
        assert ks == {k for k in SEAM_BLOCKS if k <= top}, (c, ks)
    assert any(k == 1024 and s[:2] == ("head_last", 1) for a in seam_plan(mnp.BLOCK_SIZES[1]) for k, s in a), "the one-candidate block is a lead piece"
    assert any(k == 1023 and s[:2] == ("head_last", 1024) for a in seam_plan(mnp.BLOCK_SIZES[0]) for k, s in a), "a block without a head ends the data"


# ---- the 8.4 M-record layouts: each uploaded once and shared ------------------------------------------------------------------------
class _Uploaded:
    """The layout in use: its records on the host, and on the device in an arena of their own at the skew asked for."""

    def __init__(self, ia, ctx):
        self.ia, self.ctx, self.key, self.ar = ia, ctx, None, None

    def get(self, name, skew, build):
        if self.key != (name, skew):
            self.release()
            built = build()
            self.recs, self.extra = built if isinstance(built, tuple) else (built, None)
            n = len(self.recs)
            self.ar = _arena(self.ia, self.ctx, 24 * n)
            self.d = self.ar.carve(24 * n, skew)
            self.d.upload(self.recs)
            self.heads = None
            self.key = (name, skew)
        return self.recs, self.d

    def settle(self, what):
        """After a case: the guard zones, and the records are read only."""
        self.ar.check(what)
        n = len(self.recs)
        assert np.array_equal(self.d.download(count=24 * n), np.ascontiguousarray(self.recs).view(np.uint8)), "the records are read only"

    def release(self):
        if self.ar is not None:
            self.ar.free()
        self.key = self.ar = self.recs = self.d = self.heads = self.extra = None


@pytest.fixture(scope="module")
def big(ia, ctx):
    b = _Uploaded(ia, ctx)
    yield b
    b.release()


# ---- 2. saturation: stitch seams -------------------------------------------------------------------------------------------------
MIXED_SEED, MIXED_FIRST_ROW = 0x32B00, 127


@pytest.mark.parametrize("skew", SKEWS)
def test_stitch_matches_numpy(ia, ctx, big, skew):
    n = BIG_N
    recs, d = big.get("mixed", skew, lambda: snp.stitch_mixed(n))
    heads = snp.head_positions(recs)
    head, nseg = _plan(n, skew)
    per_seg = [np.bincount((np.maximum(p - head, -1) // SEG + 1).astype(np.int64), minlength=nseg - 1) for p in heads]
    for c, least in zip(per_seg, ((100, 100, 50), (20, 50, 100))):   # tiled segments without a head, with one, with several: at both depths
        have = [int((c[1:-1] == 0).sum()), int((c[1:-1] == 1).sum()), int((c[1:-1] > 1).sum())]
        assert all(x > y for x, y in zip(have, least)), have
    lengths = [np.diff(np.append(p, n)) for p in heads]
    assert lengths[0].min() > 0.29 * SEG and lengths[0].max() < 5 * SEG and lengths[1].max() > SEG and np.median(lengths[1]) < SEG / 8
    uu = snp.u(MIXED_SEED, MIXED_FIRST_ROW, n)
    m1 = np.sort(np.minimum.reduceat(uu, heads[0]))
    ts = [int(m1[k * (len(m1) // 33)]) + 1 for k in range(1, 33)]    # quantiles of the barcodes' smallest u: every bin closes len // 33 of them
    want = snp.saturation_curve_from(uu, recs, ts, heads)
    steps = np.diff(np.array([(0, 0, 0)] + [w[1:] for w in want]), axis=0)
    assert len(ts) == 32 and (steps[:, 1] >= 10).all() and (steps[:, 2] >= 10).all(), "every bin closes several runs at both depths"
    assert want[-1][2] < len(heads[0]) and want[-1][3] < len(heads[1]) // 2, "no bin is the trivial one"
    for pick in (ts, ts[16:17], ts[3::6][:5]):
        assert len(pick) in (32, 1, 5)
        got = _curve(ia, ctx, d, n, MIXED_FIRST_ROW, MIXED_SEED, pick)
        exp = [w for w in want if w[0] in pick]
        assert got == exp, (skew, len(pick), [(j, g, w) for j, (g, w) in enumerate(zip(got, exp)) if g != w][:4])
    big.settle("stitch, mixed runs")


LONE_SEED = 0x32A00                                              # (the smallest u of the middle third is the smallest of every window used: asserted)


@functools.lru_cache(maxsize=1)
def _lone():
    """-> (u of positions 0 .. 3n - 1 under LONE_SEED, g = the position of the smallest over [n, 2n), u(g))."""
    n = BIG_N
    seq = snp.u(LONE_SEED, 0, 3 * n)
    g = n + int(np.argmin(seq[n:2 * n]))
    assert int(np.argmin(seq[g - n + 1:g + n])) == n - 1, "one kept read in every window that holds g"
    return seq, g, int(seq[g])


def _stitch_layout(layout, skew):
    return snp.stitch_runs(BIG_N, skew // 8, layout, SEAM_SEGMENTS)


def _check_stitch_layout(layout, skew, recs, rows):
    """From the numpy side: the runs lie where the case says, at both depths."""
    n, head = BIG_N, skew // 8
    F = lambda j: snp.seg_first_row(head, j)
    for p in snp.head_positions(recs):
        h = np.zeros(n + 1, bool)
        h[p] = True
        if layout == "long":
            (J, r), = rows
            a, b = r[0] - 1, r[-1] + 1
            assert (a, b) == (F(200) + 5, F(1029) + 100) and h[a] and h[b] and not h[a + 1:b].any()
            assert r[1:-1] == [F(j) + e for j in (256, 512, 768, 1024, 1025) for e in (-1, 0)]
            continue
        assert [J for J, _ in rows] == list(SEAM_SEGMENTS)
        for J, r in rows:
            a, b = F(J - 2) + 5, F(J + 1) + 100
            assert h[a] and h[b] and not h[a + 1:F(J)].any() and not h[F(J) + 1:b].any() and h[F(J)] == (layout == "head_on_seam")
            assert r == ([F(J) - 1, F(J)] if layout == "head_on_seam" else [a + 1, F(J) - 1, F(J), b - 1])


@pytest.mark.parametrize("layout,skew", [(l, s) for s in SKEWS for l in ("through", "head_on_seam", "long")])
def test_one_kept_read_across_stitch_seams(ia, ctx, big, layout, skew):
    """One read is kept at u(g) + 1 and none at u(g); first_row = g - r puts it on row r.  The curve is then exactly (1, 1, 1) and
    (0, 0, 0): a carry the stitch drops shows as 0 runs, one it doubles as 2.  (A wave that picks up its own aggregate in place of
    the waves' in front of it moves the kept run from the first head behind the wave seam to the first head of the wave in front:
    still one run.  That error shows where the waves in between have no head — the long layout — and in test_stitch_matches_numpy.)"""
    n = BIG_N
    seq, g, ug = _lone()
    recs, d = big.get(layout, skew, lambda: _stitch_layout(layout, skew))
    rows = big.extra
    if big.heads is None:
        _check_stitch_layout(layout, skew, recs, rows)
        big.heads = snp.head_positions(recs)
    p1 = big.heads[0]
    want = [(ug, 0, 0, 0), (ug + 1, 1, 1, 1)]
    for J, at in rows:
        # the statement, on the rows from three barcodes in front of the case's rows to three behind them (whole runs: both cuts
        # are barcode heads); every row outside holds a larger u than u(g), whatever the window (_lone)
        lo, hi = int(p1[np.searchsorted(p1, min(at)) - 3]), int(p1[np.searchsorted(p1, max(at)) + 3])
        assert 0 < lo < min(at) - 6 and max(at) + 6 < hi < n
        for r in at:
            first_row = g - r
            assert int(seq[first_row + r]) == ug and snp.saturation_curve_from(seq[first_row + lo:first_row + hi], recs[lo:hi], [ug, ug + 1]) == want, (J, r)
            what = (layout, skew, J, r)
            assert _curve(ia, ctx, d, n, first_row, LONE_SEED, [ug + 1]) == want[1:], what
            assert _curve(ia, ctx, d, n, first_row, LONE_SEED, [ug]) == want[:1], what
            assert _curve(ia, ctx, d, n, first_row, LONE_SEED, [0, ug, ug, ug + 1, ug + 1, snp.ONES])[1:5] == [want[0]] * 2 + [want[1]] * 2, what
    big.settle("one kept read")


def test_every_stitch_seam_is_laid():
    for skew in SKEWS:
        head, nseg = _plan(BIG_N, skew)
        assert nseg == 1033
        for layout, per in (("through", 4), ("head_on_seam", 2)):
            rows = _stitch_layout(layout, skew)[1]
            assert [J for J, _ in rows] == list(SEAM_SEGMENTS) and all(len(r) == per for _, r in rows)
            for J, r in rows:                                    # the last row of segment J - 1 and the first of segment J, as the plan cuts them
                assert {head + (J - 1) * SEG - 1, head + (J - 1) * SEG} <= set(r)
        (J, r), = _stitch_layout("long", skew)[1]
        assert (r[0] - head) // SEG + 1 == 200 and (r[-1] - head) // SEG + 1 == 1029
        assert all({head + (j - 1) * SEG - 1, head + (j - 1) * SEG} <= set(r) for j in (PER_WAVE, 2 * PER_WAVE, 3 * PER_WAVE, PER_ROUND, PER_ROUND + 1))


# ---- 3. dense per-segment counts beyond 1024 segments ----------------------------------------------------------------------------------
DENSE = ("barcode_counts", "pair_counts", "classify_molecules", "call_cells")


def _barcode_counts(ia, ctx, d, n, outs, cap):
    nb, npairs = C.c_size_t(12345), C.c_size_t(12345)
    ia._check(ia.lib.ibu_barcode_counts(ctx._c, _p(d), n, *[_p(o) for o in outs], cap, C.byref(nb), C.byref(npairs), None))
    return nb.value, npairs.value


def _check_dense_layout(recs, skew):
    """Per-segment barcode heads: at most 32 in the segments named (the emit pass serves them from the stash), more in every other
    full segment (it walks them), and unequal from segment to segment."""
    head, nseg = _plan(len(recs), skew)
    starts = np.flatnonzero(np.concatenate([[True], cnp._words(recs)[1:, 0] != cnp._words(recs)[:-1, 0]]))
    per_seg = np.bincount(np.maximum(starts - head, -1) // SEG + 1, minlength=nseg - 1)
    named = np.zeros(len(per_seg), bool)
    named[list(cnp.STASH_SEGMENTS)] = True
    assert len(cnp.STASH_SEGMENTS) == 40 and {255, 256, 257, 1023, 1024, 1025} <= set(cnp.STASH_SEGMENTS)
    assert (per_seg[named] <= cnp.STASH_HEADS).all() and (per_seg[named] == 0).sum() == 2 and len(set(per_seg[named].tolist())) > 20
    assert (per_seg[1:1031][~named[1:1031]] > 20 * cnp.STASH_HEADS).all() and len(set(per_seg[1:1031].tolist())) > 100
    assert all(named[j] != named[j + 1] for j in (99, 100, 101, 102, 103, 104, 105)), "stash and walk alternate"


@pytest.mark.parametrize("skew,what", [(s, w) for s in SKEWS for w in DENSE])
def test_dense_counts_beyond_1024_segments(ia, ctx, big, skew, what):
    n = BIG_N
    recs, d = big.get("dense", skew, lambda: cnp.dense_runs(n, skew // 8))
    if what == "barcode_counts":
        _check_dense_layout(recs, skew)
        want = cnp.barcode_counts(recs)
        k, pairs = len(want[0]), int(want[2].sum())
        assert k > 1_000_000 and pairs > 2 * k
        ar = _arena(ia, ctx, *[8 * k] * 3)
        try:
            outs = [ar.carve(8 * k, s) for s in (0, 8, skew)]
            assert _barcode_counts(ia, ctx, d, n, [None] * 3, 0) == (k, pairs), "size query"
            assert _barcode_counts(ia, ctx, d, n, outs[:2] + [None], k) == (k, pairs), "without unique UMIs"
            ar.check("barcode_counts without unique UMIs")
            assert _same(_download(outs[:2], k), want[:2]) and (outs[2].download(np.uint8, 8 * k) == PATTERN).all()
            assert _barcode_counts(ia, ctx, d, n, outs, k) == (k, pairs)
            ar.check("barcode_counts")
            got = _download(outs, k)
            bad = [int(np.flatnonzero(g != w)[0]) for g, w in zip(got, want) if (g != w).any()]
            assert not bad, f"first wrong entry {bad} of {k}"
        finally:
            ar.free()
    elif what == "pair_counts":
        want = cnp.pair_counts(recs)
        k, triples = len(want[0]), int(want[3].sum())
        assert k > 2_000_000 and triples > 2 * k
        ar = _arena(ia, ctx, *[8 * k] * 4)
        try:
            outs = [ar.carve(8 * k, s) for s in (skew, 0, 8, skew)]
            assert _pair_counts(ia, ctx, d, n, outs[:3] + [None], k) == (k, triples), "without distinct thirds"
            ar.check("pair_counts without distinct thirds")
            assert _same(_download(outs[:3], k), want[:3]) and (outs[3].download(np.uint8, 8 * k) == PATTERN).all()
            assert _pair_counts(ia, ctx, d, n, outs, k) == (k, triples)
            ar.check("pair_counts")
            got = _download(outs, k)
            bad = [int(np.flatnonzero(g != w)[0]) for g, w in zip(got, want) if (g != w).any()]
            assert not bad, f"first wrong entry {bad} of {k}"
        finally:
            ar.free()
    else:
        if what == "classify_molecules":
            tie_first = skew == 8
            cls, tot = mnp.classify(recs, tie_first)
            assert all((cls == c).any() for c in ((0, 1) if tie_first else (0, 1, 2))) and tot["candidates"] > 4_000_000
        else:
            cls, tot = cells_np.call_cells(recs, cells_np.MIN, 3)
            assert 0.2 < tot["cells"] / tot["barcodes"] < 0.8
        ar = _arena(ia, ctx, n)
        try:
            d_class = ar.carve(n, 3 if skew else 0)
            if what == "classify_molecules":
                got = _classify(ia, ctx, d, n, ia.MOLECULES_TIE_FIRST if tie_first else 0, d_class)
            else:
                got = _call_cells(ia, ctx, d, n, cells_np.MIN, 3, 0, d_class)
            ar.check(what)
            assert got == tot, (got, tot)
            have = d_class.download(np.uint8, n)
            bad = np.flatnonzero(have != cls)
            assert bad.size == 0, f"{bad.size} class bytes differ, first at row {int(bad[0])}: {int(have[bad[0]])} for {int(cls[bad[0]])}"
        finally:
            ar.free()
    big.settle(f"dense {what}")
