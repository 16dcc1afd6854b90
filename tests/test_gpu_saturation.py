"""Read subsampling and the saturation curve on the device (ibu_subsample_class, ibu_saturation_curve): every comparison is exact
against the numpy statement of the semantics in tests/saturation_np.py; every call goes through the C ABI, and every buffer —
d_class at exactly n bytes too — is carved at its contract size out of an arena with guard zones (the pattern of
tests/test_gpu_count.py).  The records are compared after every case: they are never written."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import count_np
from tests import saturation_np as snp
from tests.test_gpu_count import PATTERN, _arena, _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [0, 1, 2, 63, 127, 128, 129, 255, 2559, 2561, 100_003, 1_000_003]
SEG, TILE = 8192, 128                                            # runs_walk.hpp: records per segment / per tile
SEAM_ROWS = [(SEG * k, d) for k in (1, 2, 12) for d in (-1, 0, 1)] + [(TILE * k, d) for k in (3, 63, 65) for d in (-1, 0, 1)]
NS = SIZES + [s + d for s, d in SEAM_ROWS]
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
SHAPES = ["own_run", "one_run", "threes", "seam", "span", "random"]
BIG = 1_000_003
# the grid: every size x skew x shape, but above 1e5 records only own_run and random, and the run that spans three segments only
# where three segments exist
GRID = [(n, skew, shape) for n, skew, shape in itertools.product(NS, SKEWS, SHAPES)
        if (n < BIG or shape in ("own_run", "random")) and (shape != "span" or n > 4 * SEG)]
assert len(set(NS)) == len(NS) == 30 and len(GRID) == 2 * (29 * 5 + 4 + 2), len(GRID)
GARBAGE = 0x5A5A5A5A5A5A5A5A
ONES = snp.ONES
FIRST_ROWS = [0, 1, 127, (1 << 40) + 3]
SEEDS = [0, 1, 0x32300, ONES]


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _curve(ia, ctx, d, n, first_row, seed, ts, stream=None):
    """One ibu_saturation_curve call through the C ABI -> [(threshold, reads, barcodes, molecules)]."""
    from ibu_amd import _lib
    k = len(ts)
    pts = (_lib.CSaturationPoint * k)(*[_lib.CSaturationPoint(*[GARBAGE] * 4) for _ in range(k)])
    ia._check(ia.lib.ibu_saturation_curve(ctx._c, _p(d), n, first_row, seed, (C.c_uint64 * k)(*ts), k, pts, stream))
    return [tuple(int(getattr(p, f)) for f in snp.FIELDS) for p in pts]


def _subsample(ia, ctx, n, first_row, seed, t, d_class, want_kept=True, stream=None):
    k = C.c_size_t(GARBAGE)
    ia._check(ia.lib.ibu_subsample_class(ctx._c, n, first_row, seed, t, _p(d_class), C.byref(k) if want_kept else None, stream))
    return k.value if want_kept else None


def _threes(n):
    """Molecules of three records, barcodes of six."""
    r = np.zeros(n, snp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    w[:, 0], w[:, 1], w[:, 2] = i // np.uint64(6), (i // np.uint64(3)) & np.uint64(1), 1
    return r, w


def _seam_rows(n, head, d=None):
    """The rows head + s + d next to a tile or segment boundary that lie inside n records (d: one of -1, 0, 1, or all three)."""
    return sorted({head + s + dd for s, dd in SEAM_ROWS if (d is None or dd == d) and 0 <= head + s + dd < n})


def _seam(n, head, d):
    """Runs of three, and at every seam row head + s + d that fits a run of ten records that ends just in front of the row and one
    of two records that begins on it — at both depths."""
    r, w = _threes(n)
    laid = []
    for k, row in enumerate(_seam_rows(n, head, d)):
        big = (1 << 40) + 2 * k
        if row - 10 < 0 or row + 2 > n:
            continue
        w[row - 10:row, 0], w[row - 10:row, 1] = big, 4
        w[row:row + 2, 0], w[row:row + 2, 1] = big + 1, 5
        laid.append(row)
    return r, laid


def _span(n, head):
    """Runs of three, and one barcode from just in front of the second segment to just behind the fourth: its first 8192 records one
    molecule, the rest another."""
    r, w = _threes(n)
    a, b = head + SEG - 6, head + 4 * SEG + 9
    w[a:b, 0], w[a:b, 1] = 1 << 41, (np.arange(b - a) >= SEG).astype(np.uint64)
    return r


@functools.lru_cache(maxsize=4)
def _shape(shape, n, skew, d=0):
    r = np.zeros(n, snp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    head = min(skew // 8, n)
    if shape == "own_run":
        w[:, 0], w[:, 1], w[:, 2] = i, 7, 9
    elif shape == "one_run":
        w[:, 0], w[:, 1], w[:, 2] = 5, 7, i
    elif shape == "threes":
        r = _threes(n)[0]
    elif shape == "seam":
        r = _seam(n, head, d)[0]
    elif shape == "span":
        r = _span(n, head)
    else:                                                        # sorted random records over a small alphabet: runs of ~50 and ~10
        rng = np.random.default_rng(0x32400 + n)
        w[:, 0], w[:, 1], w[:, 2] = rng.integers(0, n // 50 + 1, n), rng.integers(0, 5, n), rng.integers(0, 3, n)
        r = count_np.sort_records(r)
    assert len(r) == n
    return r


def _threshold_lists(n, head, seed, first_row):
    """k = 1, 5 and 32: 0, all ones, duplicates, 2^63, 2^64 / 4096, and u(row), u(row) + 1 for rows on seams."""
    uu = snp.u(seed, first_row, n)
    rows = ([r for r in (_seam_rows(n, head) + [0, n - 1]) if 0 <= r < n] or [0])[-6:]
    at = [int(uu[r]) for r in rows] if n else [12345]
    one = [[1 << 63], [ONES], [0], [at[0] + 1]][(n + head) % 4]
    five = sorted([0, at[-1], at[-1] + 1, 1 << 63, ONES])
    pool = [0, 0, 1 << 52, 1 << 63, 1 << 63, ONES, ONES] + [x + e for x in at for e in (0, 1)]
    rng = np.random.default_rng(n + 7)
    pool += [2 * int(x) for x in rng.integers(0, 1 << 63, 32)]
    return [one, five, sorted(min(x, ONES) for x in pool[:32])]


def _check_case(ia, ctx, recs, n, skew):
    ar = _arena(ia, ctx, 24 * n)
    try:
        d = ar.carve(24 * n, skew)
        if n:
            d.upload(recs)
        head = min(skew // 8, n)
        for j in range(3):
            seed, first_row = SEEDS[(n + j) % 4], FIRST_ROWS[(n // 2 + j + skew) % 4]
            for ts in _threshold_lists(n, head, seed, first_row):
                got = _curve(ia, ctx, d, n, first_row, seed, ts)
                want = snp.saturation_curve(recs, seed, first_row, ts)
                assert got == want, (f"seed {seed} first_row {first_row} k {len(ts)}", [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:4])
        ar.check("saturation_curve")
        assert n == 0 or d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
    finally:
        ar.free()


@pytest.mark.parametrize("n,skew,shape", GRID)
def test_saturation_curve_matches_numpy(ia, ctx, n, skew, shape):
    for d in ((-1, 0, 1) if shape == "seam" and n > TILE * 3 else (0,)):
        _check_case(ia, ctx, _shape(shape, n, skew, d), n, skew)


def test_the_shapes_have_what_they_claim():
    for d in (-1, 0, 1):
        for head in (0, 1):
            recs, laid = _seam(100_003, head, d)
            assert laid == [head + s + d for s in sorted({s for s, _ in SEAM_ROWS})], (d, laid)
            w = count_np._words(recs)
            for row in laid:
                assert w[row, 0] != w[row - 1, 0] and w[row - 1, 0] == w[row - 10, 0] != w[row - 11, 0] and w[row + 1, 0] == w[row, 0] != w[row + 2, 0]
    recs = _shape("span", 100_003, 8)
    first, second, reads, _ = count_np.pair_counts(recs)
    long = np.flatnonzero(first == np.uint64(1 << 41))
    start = int(np.concatenate([[0], np.cumsum(reads)])[long[0]])
    assert reads[long].tolist() == [SEG, 2 * SEG + 15] and start == 1 + SEG - 6, "from in front of the second segment to behind the fourth"
    assert set(count_np.pair_counts(_shape("threes", 2561, 0))[2][:-1].tolist()) == {3}
    assert len(count_np.pair_counts(_shape("one_run", 2561, 0))[0]) == 1 and len(count_np.pair_counts(_shape("own_run", 2561, 0))[0]) == 2561
    reads = count_np.pair_counts(_shape("random", 100_003, 0))[2]
    assert 5 < reads.mean() < 20 and reads.max() > 20


# ---- one kept read at every seam: a dropped or doubled carry shows as 0 or 2 ------------------------------------------------------
LONE_N = 100_003
LONE_SEED = 0x32500


@functools.lru_cache(maxsize=1)
def _lone_read():
    """-> (g, u(g)): the row of the smallest u over positions [BIG, 2^22 - BIG) under LONE_SEED."""
    uu = snp.u(LONE_SEED, 0, 1 << 22)
    g = BIG + int(np.argmin(uu[BIG:(1 << 22) - BIG]))
    return g, int(uu[g])


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("shape", ["span", "one_run", "seam"])
def test_one_kept_read_at_every_seam(ia, ctx, shape, skew):
    n, head = LONE_N, skew // 8
    g, ug = _lone_read()
    rows = _seam_rows(n, head)
    assert len(rows) == 18
    ar = _arena(ia, ctx, 24 * n)
    try:
        d = ar.carve(24 * n, skew)
        for dd in ((-1, 0, 1) if shape == "seam" else (0,)):
            recs = _shape(shape, n, skew, dd)
            d.upload(recs)
            for r in rows:
                first_row = g - r
                # from the statement, before the device is asked: exactly one read is kept at u(g) + 1, it sits on row r, and none at u(g)
                cls, kept = snp.subsample_class(n, LONE_SEED, first_row, ug + 1)
                assert kept == 1 and cls[r] == snp.KEPT and snp.subsample_class(n, LONE_SEED, first_row, ug)[1] == 0
                want = [(ug, 0, 0, 0), (ug + 1, 1, 1, 1)]
                assert snp.saturation_curve(recs, LONE_SEED, first_row, [ug, ug + 1]) == want
                assert _curve(ia, ctx, d, n, first_row, LONE_SEED, [ug + 1]) == want[1:], (shape, skew, dd, r)
                assert _curve(ia, ctx, d, n, first_row, LONE_SEED, [ug]) == want[:1], (shape, skew, dd, r)
                assert _curve(ia, ctx, d, n, first_row, LONE_SEED, [0, ug, ug, ug + 1, ug + 1, ONES])[1:5] == [want[0]] * 2 + [want[1]] * 2
            assert d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
        ar.check("one kept read")
    finally:
        ar.free()


# ---- the subsample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_subsample_class_matches_numpy(ia, ctx, n):
    ar = _arena(ia, ctx, n, n, n, n)
    try:
        bufs = [ar.carve(n, skew) for skew in (0, 3, 8, 13)]       # d_class at exactly n bytes, at four alignments
        pattern = np.full(n, PATTERN, np.uint8).tobytes()
        for j, d_class in enumerate(bufs):
            seed, first_row = SEEDS[(n + j) % 4], FIRST_ROWS[(n + j) % 4]
            uu = snp.u(seed, first_row, max(n, 1))
            for t in dict.fromkeys([1 << 63, 0, ONES, 1 << 52, int(uu[n // 2]), min(int(uu[n // 2]) + 1, ONES), int(uu[max(n, 1) - 1]) + 1]):
                if n >= BIG and t not in (1 << 63, ONES):
                    continue
                t = min(t, ONES)
                cls, kept = snp.subsample_class(n, seed, first_row, t)
                what = f"n {n} buffer {j} seed {seed} first_row {first_row} t {t:#x}"
                assert _subsample(ia, ctx, n, first_row, seed, t, d_class) == kept, what
                if n:
                    have = d_class.download(np.uint8, n)
                    bad = np.flatnonzero(have != cls)
                    assert bad.size == 0, f"{what}: {bad.size} class bytes differ, first at row {int(bad[0])}"
                # the count alone: nothing is written
                d_class.upload(np.full(max(n, 1), PATTERN, np.uint8)[:n]) if n else None
                assert _subsample(ia, ctx, n, first_row, seed, t, None) == kept, what
                assert n == 0 or d_class.download(np.uint8, n).tobytes() == pattern
                # the classes alone: asynchronous, right after a synchronisation
                assert _subsample(ia, ctx, n, first_row, seed, t, d_class, want_kept=False) is None
                ctx.synchronize()
                assert n == 0 or d_class.download(np.uint8, n).tobytes() == cls.tobytes(), what
            ar.check(f"subsample_class n {n} buffer {j}")
    finally:
        ar.free()


# ---- agreement with the code that exists: subsample -> select -> the run counts of the subset -------------------------------------
@pytest.mark.parametrize("shape,n,skew", [("random", 100_003, 0), ("span", 100_003, 8), ("seam", 2561, 8), ("threes", 8193, 0), ("one_run", 24_577, 8),
                                          ("own_run", 1_000_003, 0)])
def test_every_point_is_what_subsample_select_and_the_run_counts_give(ia, ctx, shape, n, skew):
    recs = _shape(shape, n, skew)
    seed, first_row = 0x32600 + n, 127
    uu = snp.u(seed, first_row, n)
    ts = sorted([0, 1 << 60, int(uu[SEG if n > SEG else n // 2]) + 1, 1 << 63, 3 << 62, ONES])
    ar = _arena(ia, ctx, 24 * n, 24 * n, n)
    try:
        d, out, d_class = ar.carve(24 * n, skew), ar.carve(24 * n, 8 - skew), ar.carve(n, 5)
        d.upload(recs)
        curve = _curve(ia, ctx, d, n, first_row, seed, ts)
        assert curve == snp.saturation_curve(recs, seed, first_row, ts)
        for t, reads, barcodes, molecules in curve:
            assert _subsample(ia, ctx, n, first_row, seed, t, d_class) == reads
            k = C.c_size_t()
            ia._check(ia.lib.ibu_select_records(ctx._c, _p(d), _p(d_class), n, 1 << ia.SAMPLE_KEPT, _p(out), n, C.byref(k), None))
            assert k.value == reads
            npairs, ntriples, nb, nbu = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
            ia._check(ia.lib.ibu_pair_counts(ctx._c, _p(out), reads, None, None, None, None, 0, C.byref(npairs), C.byref(ntriples), None))
            ia._check(ia.lib.ibu_barcode_counts(ctx._c, _p(out), reads, None, None, None, 0, C.byref(nb), C.byref(nbu), None))
            # (no key returns in these shapes: a run of the subset is a run of the input with a kept read)
            assert (npairs.value, nb.value) == (molecules, barcodes), (hex(t), reads)
            assert nbu.value == npairs.value
        ar.check("subsample -> select -> counts")
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        ar.free()


def test_unsorted_input_is_the_run_level_answer(ia, ctx):
    n = 100_003
    recs = _shape("random", n, 0)[np.random.default_rng(0x32700).permutation(n)]
    assert len(count_np.pair_counts(recs)[0]) > 5 * len(count_np.pair_counts(_shape("random", n, 0))[0])
    _check_case(ia, ctx, recs, n, 8)


def test_forms_of_the_call(ia, ctx):
    from ibu_amd import _lib
    n = 100_003
    recs = _shape("random", n, 0)
    seed, first_row = 7, 1
    ts = [snp.sample_threshold(f) for f in (0.1, 0.25, 0.5, 0.5, 1)]
    want = snp.saturation_curve(recs, seed, first_row, ts)
    ar = _arena(ia, ctx, 24 * n, n)
    other, fresh = ia.Context(0), ia.Context(0)
    try:
        d, d_class = ar.carve(24 * n, 8), ar.carve(n, 1)
        d.upload(recs)
        pattern = np.full(n, PATTERN, np.uint8).tobytes()
        # every invalid argument is refused before anything is touched, the points included
        up, down = (C.c_uint64 * 33)(*range(33)), (C.c_uint64 * 3)(1, 3, 2)
        pts = (_lib.CSaturationPoint * 33)(*[_lib.CSaturationPoint(*[GARBAGE] * 4) for _ in range(33)])
        bad = [(d, n, up, 0, pts), (d, n, up, 33, pts), (d, n, down, 3, pts), (d, n, None, 1, pts), (d, n, up, 1, None), (None, 1, up, 1, pts),
               (ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 24), 1, up, 1, pts), (d, 1 << 40, up, 1, pts), (d, 0, up, 0, pts), (d, 0, down, 3, pts)]
        for j, (buf, count, tarr, k, p) in enumerate(bad):
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_saturation_curve(ctx._c, _p(buf), count, 0, 0, tarr, k, p, None))
            assert ei.value.kind == "InvalidArg", j
            assert all(getattr(q, f) == GARBAGE for q in pts for f in snp.FIELDS), (j, "the points of a refused call are untouched")
        kept = C.c_size_t(GARBAGE)
        for count, cls, kp in ((1 << 40, d_class, C.byref(kept)), (n, None, None), (0, None, None)):
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_subsample_class(ctx._c, count, 0, 0, 1 << 63, _p(cls), kp, None))
            assert ei.value.kind == "InvalidArg" and kept.value == GARBAGE
        ar.check("refused calls")
        assert d_class.download(np.uint8, n).tobytes() == pattern, "a refused call writes nothing"
        # n == 0: every point is {threshold, 0, 0, 0}, with or without records; the subsample touches nothing
        assert _curve(ia, ctx, None, 0, 5, 6, ts) == _curve(ia, ctx, d, 0, 5, 6, ts) == [(t, 0, 0, 0) for t in ts]
        assert _subsample(ia, ctx, 0, 0, 0, ONES, d_class) == 0 and _subsample(ia, ctx, 0, 0, 0, ONES, None) == 0
        assert _subsample(ia, ctx, 0, 0, 0, ONES, d_class, want_kept=False) is None
        ar.check("n == 0")
        assert d_class.download(np.uint8, n).tobytes() == pattern
        # a second call on the same context and scratch, after a larger one, gives what a fresh context gives
        assert _curve(ia, ctx, d, n, first_row, seed, ts) == want
        small = 2561
        small_want = snp.saturation_curve(recs[:small], seed, first_row, ts)
        assert _curve(ia, ctx, d, small, first_row, seed, ts) == small_want == _curve(ia, fresh, d, small, first_row, seed, ts)
        assert _curve(ia, ctx, d, n, first_row, seed, ts) == want
        # on a stream of another context
        assert _curve(ia, ctx, d, n, first_row, seed, ts, stream=other.stream) == want
        cls, k = snp.subsample_class(n, seed, first_row, ts[2])
        assert _subsample(ia, ctx, n, first_row, seed, ts[2], d_class, stream=other.stream) == k
        assert d_class.download(np.uint8, n).tobytes() == cls.tobytes()
        ar.check("streams")
        # the Python wrapper
        got = ctx.saturation_curve(d, n, fractions=(0.1, 0.25, 0.5, 0.5, 1), seed=seed, first_row=first_row)
        assert got == [ia.SaturationPoint(*w) for w in want] and got[-1].reads == n
        assert ctx.saturation_curve(d, n, thresholds=ts, seed=seed, first_row=first_row) == got
        buf, kk = ctx.subsample_class(n, fraction=0.5, seed=seed, first_row=first_row)
        assert kk == k and buf.download(np.uint8, n).tobytes() == cls.tobytes()
        assert ctx.subsample_class(n, False, threshold=ts[2], seed=seed, first_row=first_row) == (None, k)
        buf2, none = ctx.subsample_class(n, buf, fraction=1, count=False)
        ctx.synchronize()
        assert none is None and buf2 is buf and not buf.download(np.uint8, n).any()
        out, kept_n = ctx.select_records(d, ctx.subsample_class(n, buf, fraction=0.5, seed=seed, first_row=first_row)[0], n, 1 << ia.SAMPLE_KEPT)
        ctx.synchronize()
        assert kept_n == k and out.download(snp.REC, k).tobytes() == recs[cls == snp.KEPT].tobytes(), "the subset, in input order"
        buf.free()
        out.free()
        with pytest.raises(ValueError):
            ctx.saturation_curve(d, n, fractions=[0.5, 0.25])
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        other.close()
        fresh.close()
        ar.free()


def test_count_file_saturation_and_subsample(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len, n, K, seed = 16, 20_011, 4, 9
    rng = np.random.default_rng(0x32800)
    recs = np.zeros(n, snp.REC)
    recs["barcode"], recs["umi"], recs["index"] = rng.integers(0, 40, n), rng.integers(0, 200, n), rng.integers(0, 3, n)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    text = lambda c: "".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(bc_len))
    s = count_np.sort_records(recs)
    thresholds = [ONES if j == K else (j << 64) // K for j in range(1, K + 1)]

    def lines(sub):
        curve = snp.saturation_curve(sub, 0, 0, thresholds)
        sat = [f"#saturation\t{(j + 1) / K:.6f}\t{r}\t{b}\t{m}\t{(1 - m / r if r else 0):.6f}" for j, (_, r, b, m) in enumerate(curve)]
        b, i, reads, umis = count_np.brute_force_matrix(sub)
        return sat, [f"{text(bb)}\t{ii}\t{uu}\t{rr}" for bb, ii, rr, uu in zip(b.tolist(), i.tolist(), reads.tolist(), umis.tolist())]

    r = subprocess.run([str(exe), f"--saturation={K}", str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sat, matrix = lines(s)
    out = r.stdout.splitlines()
    assert out[:K] == sat and [l for l in out if not l.startswith("#")] == matrix
    assert float(sat[-1].split("\t")[-1]) > 0.3 and sat[-1].split("\t")[2] == str(n), "a curve worth the name: well saturated at full depth"
    cls, kept = snp.subsample_class(n, seed, 0, 1 << 63)
    r = subprocess.run([str(exe), f"--subsample=0.5:{seed}", f"--saturation={K}", str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sat, matrix = lines(s[cls == snp.KEPT])
    out = r.stdout.splitlines()
    assert out[:K] == sat and [l for l in out if not l.startswith("#")] == matrix
    assert f"{n} records: subsample 0.5 seed {seed}; kept {kept}" in r.stderr
