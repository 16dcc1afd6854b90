"""The merge of sorted records on the device (ibu_merge_sorted, ibu_merge_sorted_runs): every comparison is byte for byte against
the numpy statement of the semantics in tests/merge_np.py, every call goes through the C ABI, and every buffer is carved at exactly
its contract size out of an arena with guard zones (the pattern of tests/test_gpu_count.py).  The cases of one shape share one
arena: one upload, one guard check and one download for all size pairs."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import merge_np as mnp
from tests.count_np import REC
from tests.test_gpu_count import Arena, GUARD, PATTERN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 256                                                          # k_merge.hip / kernels.h kMergeTile: records per output tile
SMALL = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 5 * T + 3]
PAIRS = list(itertools.product(SMALL, SMALL)) + [(100_003, 30_011)]
BIG = (1_000_003, 300_007)
SHAPES = ["a_below_b", "b_below_a", "interleave", "identical", "tie_run", "w2_only", "w0_low", "w0_high", "top_bit", "few", "random"]
SKEWS = list(itertools.product([0, 8], repeat=3))
SKEW_PAIRS = [(0, T + 1), (1, 1), (T - 1, T + 1), (T + 1, T - 1), (65, 2 * T + 1), (5 * T + 3, T), (2 * T + 1, 2 * T - 1)]
assert len(PAIRS) == 145 and len(SKEWS) == 8


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _p(buf):
    return C.c_void_p(buf.ptr) if buf is not None else None


def _merge(ia, ctx, a, na, b, nb, out, src=None, stream=None):
    ia._check(ia.lib.ibu_merge_sorted(ctx._c, _p(a), na, _p(b), nb, _p(out), _p(src), stream))


def _merge_runs(ia, ctx, recs, tmp, lengths, stream=None):
    arr = (C.c_size_t * max(len(lengths), 1))(*lengths)
    ia._check(ia.lib.ibu_merge_sorted_runs(ctx._c, _p(recs), _p(tmp), arr, len(lengths), stream))


def _recs(w0, w1=0, w2=0):
    w0 = np.asarray(w0, np.uint64)
    r = np.zeros(len(w0), REC)
    r["barcode"], r["umi"], r["index"] = w0, w1, w2
    return r


def _sort(r):
    w = np.ascontiguousarray(r).view(np.uint64).reshape(-1, 3)
    return np.ascontiguousarray(w[np.lexsort((w[:, 2], w[:, 1], w[:, 0]))]).view(REC).reshape(-1)


def _shape(shape, na, nb, seed=0):
    """Two sorted inputs of na and nb records."""
    i, j = np.arange(na, dtype=np.uint64), np.arange(nb, dtype=np.uint64)
    rng = np.random.default_rng(0x3E6E00 + 7919 * na + nb + seed)
    if shape == "a_below_b":                                     # tiles fed by one input only, both search endpoints
        return _recs(i), _recs(j + np.uint64(na))
    if shape == "b_below_a":
        return _recs(i + np.uint64(nb)), _recs(j)
    if shape == "interleave":
        return _recs(2 * i), _recs(2 * j + np.uint64(1))
    if shape == "identical":                                     # the source bytes must be na zeros, then nb ones
        return _recs(np.full(na, 5, np.uint64), 6, 7), _recs(np.full(nb, 5, np.uint64), 6, 7)
    if shape == "tie_run":                                       # one key: the last three quarters of a and the first three quarters of b
        k = np.uint64(1 << 40)
        return _recs(np.where(i < na // 4, i, k)), _recs(np.where(j < nb - nb // 4, k, k + np.uint64(1) + j))
    if shape == "w2_only":
        return _recs(np.full(na, 9, np.uint64), 9, 2 * i), _recs(np.full(nb, 9, np.uint64), 9, 2 * j + np.uint64(1))
    if shape == "w0_low":                                        # only the low 32 bits of w0 differ
        hi = np.uint64(5 << 32)
        return _recs(hi + 2 * i, 3, 3), _recs(hi + 2 * j + np.uint64(1), 3, 3)
    if shape == "w0_high":                                       # only the high 32 bits of w0 differ
        return _recs(((2 * i) << np.uint64(32)) + np.uint64(7), 3, 3), _recs(((2 * j + np.uint64(1)) << np.uint64(32)) + np.uint64(7), 3, 3)
    if shape == "top_bit":                                       # values at and above 2^63 in every word: a signed compare puts them first
        top = np.uint64(1 << 63)
        a = _recs(2 * i + np.where(i >= na // 2, top, np.uint64(0)), top, top + i)
        b = _recs(2 * j + np.uint64(1) + np.where(j >= nb // 2, top, np.uint64(0)), top, top + j)
        return a, b
    if shape == "few":                                           # eight distinct records
        keys = rng.integers(0, 2**64, (8, 3), dtype=np.uint64, endpoint=False)
        pick = lambda n: _sort(np.ascontiguousarray(keys[rng.integers(0, 8, n)]).view(REC).reshape(-1))
        return pick(na), pick(nb)
    assert shape == "random"
    full = lambda n: _sort(np.ascontiguousarray(rng.integers(0, 2**64, (n, 3), dtype=np.uint64, endpoint=False)).view(REC).reshape(-1))
    return full(na), full(nb)


def _is_sorted(r):
    w = np.ascontiguousarray(r).view(np.uint64).reshape(-1, 3).astype(object)
    return all(tuple(w[k]) <= tuple(w[k + 1]) for k in range(0, len(w) - 1, max(1, len(w) // 2000)))


class Case:
    def __init__(self, ar, a, b, skews=(0, 0, 0), want_src=True):
        self.a, self.b, self.na, self.nb = a, b, len(a), len(b)
        n = self.na + self.nb
        self.da, self.db = ar.carve(24 * self.na, skews[0]), ar.carve(24 * self.nb, skews[1])
        self.out = ar.carve(24 * n, skews[2])
        self.src = ar.carve(n, skews[2]) if want_src else None
        if self.na:
            self.da.upload(a)
        if self.nb:
            self.db.upload(b)

    def run(self, ia, ctx):
        _merge(ia, ctx, self.da, self.na, self.db, self.nb, self.out, self.src)

    def verify(self, what, want=None):
        n = self.na + self.nb
        if n == 0:
            return
        out, src = want if want is not None else mnp.merge(self.a, self.b)
        assert self.out.download(count=24 * n).tobytes() == out.tobytes(), f"{what}: records"
        if self.src is not None:
            got = self.src.download(np.uint8, n)
            assert got.tobytes() == src.tobytes(), f"{what}: source bytes, first difference at {int(np.flatnonzero(got != src)[0])}"
        assert self.na == 0 or self.da.download(count=24 * self.na).tobytes() == self.a.tobytes(), f"{what}: a is read only"
        assert self.nb == 0 or self.db.download(count=24 * self.nb).tobytes() == self.b.tobytes(), f"{what}: b is read only"


def _arena_for(ia, ctx, sizes, slack=4):
    total = sum(49 * (na + nb) for na, nb in sizes) + len(sizes) * slack * (GUARD + 512) + 2 * GUARD + 4096
    return Arena(ia, ctx, total)


# ---- every shape at every size pair -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_merge_matches_numpy_at_every_size_pair(ia, ctx, shape):
    ar = _arena_for(ia, ctx, PAIRS)
    try:
        cases = []
        for na, nb in PAIRS:
            a, b = _shape(shape, na, nb)
            cases.append(Case(ar, a, b))
        assert all(_is_sorted(c.a) and _is_sorted(c.b) for c in cases[-3:])
        if shape == "tie_run":
            c = cases[PAIRS.index((5 * T + 3, 5 * T + 3))]
            assert int((c.a["barcode"] == 1 << 40).sum()) > 2 * T and int((c.b["barcode"] == 1 << 40).sum()) > 2 * T
        for c in cases:
            c.run(ia, ctx)
        ar.check(f"merge {shape}")
        for c in cases:
            c.verify(f"{shape} {c.na}+{c.nb}")
            if shape == "identical" and c.na + c.nb:
                assert c.src.download(np.uint8, c.na + c.nb).tolist() == [0] * c.na + [1] * c.nb
    finally:
        ar.free()


@pytest.fixture(scope="module")
def big():
    """The large pair, its reference computed once: full-range keys with a tie run of 3 T records of each input in the middle."""
    na, nb = BIG
    a, b = _shape("random", na, nb)
    k = a[na // 2].copy()
    a[na // 2:na // 2 + 3 * T] = k
    b[nb // 3:nb // 3 + 3 * T] = k
    a, b = _sort(a), _sort(b)
    return a, b, mnp.merge(a, b)


@pytest.mark.parametrize("blocks_per_cu", [0, 1])
def test_merge_large_pair(ia, big, blocks_per_cu):
    """1.3 million records; with one workgroup per CU a wave sweeps more than one tile."""
    a, b, want = big
    c = ia.Context(0)
    try:
        if blocks_per_cu:
            c.set_option("blocks_per_cu", blocks_per_cu)
        ar = _arena_for(ia, c, [BIG])
        case = Case(ar, a, b)
        case.run(ia, c)
        ar.check("merge, large pair")
        case.verify(f"large pair, blocks_per_cu {blocks_per_cu}", want)
        ar.free()
    finally:
        c.close()


@pytest.mark.parametrize("skews", SKEWS)
def test_merge_at_every_phase_of_the_three_arrays(ia, ctx, skews):
    ar = _arena_for(ia, ctx, SKEW_PAIRS * 2)
    try:
        cases = [Case(ar, *_shape(shape, na, nb, seed=1), skews=skews) for shape in ("random", "tie_run") for na, nb in SKEW_PAIRS]
        for c in cases:
            c.run(ia, ctx)
        ar.check(f"merge, skews {skews}")
        for c in cases:
            c.verify(f"skews {skews} {c.na}+{c.nb}")
    finally:
        ar.free()


# ---- one record against many ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True])
def test_single_record_lands_at_its_stable_position(ia, ctx, swapped):
    m = 3 * T
    spots = [0, T - 1, T, T + 1, m]                              # m = na + nb - 1
    ar = _arena_for(ia, ctx, [(1, m)] * len(spots))
    try:
        cases = []
        for p in spots:
            if not swapped:                                      # a = one record equal to many[p]: it goes in front of it
                many = _recs(2 * np.arange(m, dtype=np.uint64))
                one = _recs([2 * p])
                cases.append(Case(ar, one, many))
            else:                                                # b = one record equal to many[p - 1]: it goes behind it
                many = _recs(2 * np.arange(m, dtype=np.uint64) + np.uint64(2))
                one = _recs([2 * p])
                cases.append(Case(ar, many, one))
        for c in cases:
            c.run(ia, ctx)
        ar.check("single record")
        for p, c in zip(spots, cases):
            c.verify(f"single record at {p}")
            src = c.src.download(np.uint8, m + 1)
            assert int(np.flatnonzero(src == (1 if swapped else 0))[0]) == p and int((src == (1 if swapped else 0)).sum()) == 1
    finally:
        ar.free()


# ---- forms of the call ------------------------------------------------------------------------------------------------------------
def test_source_is_optional_and_inputs_may_be_one_array(ia, ctx):
    na, nb = 2 * T + 1, 5 * T + 3
    a, b = _shape("few", na, nb)
    ar = _arena_for(ia, ctx, [(na, nb), (na, nb), (nb, nb), (nb, nb)])
    try:
        with_src, without = Case(ar, a, b), Case(ar, a, b, want_src=False)
        with_src.run(ia, ctx)
        without.run(ia, ctx)
        d = ar.carve(24 * nb, 8)
        d.upload(b)
        twice, tsrc = ar.carve(48 * nb, 0), ar.carve(2 * nb, 0)
        _merge(ia, ctx, d, nb, d, nb, twice, tsrc)               # the same array merged with itself
        part = ar.carve(24 * (2 * nb - T - 5), 0)                        # inputs that overlap each other: b[0:nb] and b[T+5:nb]
        _merge(ia, ctx, d, nb, ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * (T + 5), 24 * (nb - T - 5)), nb - T - 5, part, None)
        ar.check("source optional, one array twice")
        with_src.verify("with source")
        without.verify("without source")
        want, wsrc = mnp.merge(b, b)
        assert twice.download(count=48 * nb).tobytes() == want.tobytes() and tsrc.download(np.uint8, 2 * nb).tobytes() == wsrc.tobytes()
        assert part.download(count=24 * (2 * nb - T - 5)).tobytes() == mnp.merge(b, b[T + 5:])[0].tobytes()
        # the Python wrapper
        out, src = ctx.merge_sorted(with_src.da, na, with_src.db, nb, source=True)
        ctx.synchronize()
        want, wsrc = mnp.merge(a, b)
        assert out.download(count=24 * (na + nb)).tobytes() == want.tobytes() and src.download(np.uint8, na + nb).tobytes() == wsrc.tobytes()
        out2, none = ctx.merge_sorted(with_src.da, na, with_src.db, nb)
        ctx.synchronize()
        assert none is None and out2.download(count=24 * (na + nb)).tobytes() == want.tobytes()
        for buf in (out, src, out2):
            buf.free()
    finally:
        ar.free()


def test_merge_refuses_an_output_that_overlaps_an_input(ia, ctx):
    n = 1000
    a, b = _shape("random", n, n)
    ar = _arena_for(ia, ctx, [(n, n), (n, n)])
    try:
        both = ar.carve(48 * n + 24 * 8, 0)                      # a, then b, then room for eight more records
        both.upload(np.concatenate([a, b]))
        out = ar.carve(48 * n, 0)
        before = ar.buf.download(np.uint8)
        at = lambda first, count: ia.DeviceBuffer.wrap(ctx, both.ptr + 24 * first, 24 * count)
        refused = [(at(0, n), n, at(n, n), n, at(0, 2 * n)),     # out == a
                   (at(0, n), n, at(n, n), n, at(8, 2 * n)),     # out begins inside a, ends behind b
                   (at(0, 4), 4, at(n, 4), 4, at(n + 3, 8)),     # out overlaps the last record of b only
                   (at(4, 4), 4, at(n, 4), 4, at(0, 8)),         # out ends inside a
                   (at(0, n), n, out, 0, at(n - 1, n))]          # nb == 0: a copy, but still onto its own input
        for da, na, db, nb, o in refused:
            with pytest.raises(ia.IbuError) as ei:
                _merge(ia, ctx, da, na, db, nb, o)
            assert ei.value.kind == "InvalidArg"
        for args in ((ia.DeviceBuffer.wrap(ctx, both.ptr + 4, 24), 1, at(n, 1), 1, out), (None, 1, at(n, 1), 1, out), (at(0, 1), 1, at(n, 1), 1, None),
                     (at(0, 1), 1 << 40, at(n, 1), 1, out)):
            with pytest.raises(ia.IbuError) as ei:
                _merge(ia, ctx, *args)
            assert ei.value.kind == "InvalidArg"
        ctx.synchronize()
        assert (ar.buf.download(np.uint8) == before).all(), "a refused call touches nothing"
        _merge(ia, ctx, at(0, 4), 4, at(n, 4), 4, at(4, 8))      # ranges that only touch are fine: out = records 4 .. 12 of the first array
        _merge(ia, ctx, None, 0, None, 0, None)                  # nothing to do
        ar.check("overlap")
        assert at(4, 8).download(count=24 * 8).tobytes() == mnp.merge(a[:4], b[:4])[0].tobytes()
    finally:
        ar.free()


def test_unsorted_input_stays_in_bounds_and_keeps_the_multiset(ia, ctx):
    """Bounds safety, not a fault test: the records come back as some permutation, and nothing outside the output is written."""
    rng = np.random.default_rng(0x3E6E77)
    sizes = [(3 * T + 5, 2 * T + 9), (T - 1, 4 * T), (40, 7)]
    ar = _arena_for(ia, ctx, sizes * 2)
    try:
        cases = []
        for na, nb in sizes:
            for kind in ("shuffled", "descending"):
                a, b = _shape("random" if kind == "shuffled" else "interleave", na, nb, seed=2)
                a, b = (rng.permutation(a), rng.permutation(b)) if kind == "shuffled" else (a[::-1].copy(), b[::-1].copy())
                cases.append(Case(ar, a, b))
        for c in cases:
            c.run(ia, ctx)
        ar.check("unsorted input")
        for c in cases:
            n = c.na + c.nb
            got = c.out.download(count=24 * n).view(REC)
            assert _sort(got).tobytes() == _sort(np.concatenate([c.a, c.b])).tobytes(), "a permutation of the input multiset"
            src = c.src.download(np.uint8, n)
            assert int((src == 0).sum()) == c.na and int((src == 1).sum()) == c.nb
    finally:
        ar.free()


# ---- runs -------------------------------------------------------------------------------------------------------------------------
RUNS = {1: [[10_007], [0]],
        2: [[T + 1, 10_007], [0, T - 1], [1, 0], [0, 0]],
        3: [[0, 10_007, T - 1], [T + 1, 1, 0], [0, 0, 1]],
        5: [[0, 0, T - 1, 10_007, 0], [1, T + 1, 1, T - 1, 10_007]],
        8: [[10_007, 0, T + 1, T - 1, 1, 0, 0, 10_007], [0, 1, 1, 1, T - 1, T + 1, 10_007, 0]],
        13: [[0, T - 1, 0, 0, 10_007, 1, T + 1, 10_007, 0, 1, T - 1, T + 1, 0], [1] * 13]}


@pytest.mark.parametrize("k", sorted(RUNS))
def test_merge_runs_equals_sort(ia, ctx, k):
    """Levels: k = 2 one, 3 two, 5 and 8 three, 13 four — the last level lands in d_tmp (odd) or in d_records (even); the result is
    in d_records either way."""
    rng = np.random.default_rng(0x3E6E90 + k)
    lists = RUNS[k]
    assert all(len(l) == k for l in lists)
    ar = _arena_for(ia, ctx, [(sum(l), sum(l)) for l in lists] * 2)
    try:
        jobs = []
        for j, lengths in enumerate(lists):
            n = sum(lengths)
            keys = rng.integers(0, 2**64, (50, 3), dtype=np.uint64, endpoint=False)   # 50 distinct records: ties across runs
            runs = [_sort(np.ascontiguousarray(keys[rng.integers(0, 50, m)]).view(REC).reshape(-1)) for m in lengths]
            recs = np.concatenate(runs) if n else np.zeros(0, REC)
            skew = 8 * (j & 1)
            d, tmp, d2, tmp2 = ar.carve(24 * n, skew), ar.carve(24 * n, 0), ar.carve(24 * n, skew), ar.carve(24 * n, 0)
            if n:
                d.upload(recs)
                d2.upload(recs)
            jobs.append((lengths, recs, d, tmp, d2, tmp2))
        for lengths, recs, d, tmp, d2, tmp2 in jobs:
            _merge_runs(ia, ctx, d, tmp, lengths)
            ia._check(ia.lib.ibu_sort_records(ctx._c, _p(d2), _p(tmp2), len(recs), None))
        ar.check(f"merge_runs k={k}")
        for lengths, recs, d, tmp, d2, tmp2 in jobs:
            n = len(recs)
            if n == 0:
                continue
            got = d.download(count=24 * n).tobytes()
            assert got == _sort(recs).tobytes(), lengths
            assert got == mnp.merge_runs(recs, lengths).tobytes(), lengths
            assert got == d2.download(count=24 * n).tobytes(), "what ibu_sort_records gives"
        # the Python wrapper
        lengths, recs, d, tmp = jobs[0][:4]
        if len(recs):
            d.upload(recs)
            ctx.merge_sorted_runs(d, tmp, lengths)
            ctx.synchronize()
            assert d.download(count=24 * len(recs)).tobytes() == _sort(recs).tobytes()
    finally:
        ar.free()


def test_merge_runs_argument_errors(ia, ctx):
    d, tmp = ctx.alloc(24 * 100), ctx.alloc(24 * 100)
    for lengths in ([1 << 40, 1], [(1 << 39), (1 << 39)]):
        with pytest.raises(ia.IbuError) as ei:
            _merge_runs(ia, ctx, d, tmp, lengths)
        assert ei.value.kind == "InvalidArg"
    for recs, t in ((None, tmp), (d, None), (ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 24), tmp), (d, ia.DeviceBuffer.wrap(ctx, d.ptr + 24, 24 * 50))):
        with pytest.raises(ia.IbuError) as ei:
            _merge_runs(ia, ctx, recs, t, [10, 10])
        assert ei.value.kind == "InvalidArg"
    _merge_runs(ia, ctx, None, None, [])                         # k == 0
    _merge_runs(ia, ctx, None, None, [0, 0, 0])                  # n == 0
    _merge_runs(ia, ctx, d, None, [100])                         # k == 1: nothing to do, d_tmp is not looked at
    ctx.synchronize()
    d.free()
    tmp.free()


# ---- the example ------------------------------------------------------------------------------------------------------------------
def _write(ia, path, recs, sorted_flag=True):
    h = ia.Header(16, 12)
    if sorted_flag:
        h.set_sorted()
    w = ia.Writer.from_path(str(path), h)
    w.write_batch(np.ascontiguousarray(recs))
    w.finish()
    w.close()


def test_merge_files_example(ia, tmp_path):
    from ibu_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gzutil
    exe = tmp_path / "merge_files"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merge_files.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    rng = np.random.default_rng(0x3E6EA0)
    draw = lambda n: np.ascontiguousarray(np.stack([rng.integers(0, 300, n), rng.integers(0, 64, n), rng.integers(0, 20, n)], 1).astype(np.uint64)).view(REC).reshape(-1)
    parts = [_sort(draw(n)) for n in (5_003, 20_011, 777)]
    loose = draw(3_001)
    assert not _is_sorted(loose)
    for name, r in zip("abc", parts):
        _write(ia, tmp_path / f"{name}.ibu", r)
    gzutil.bgzf_parallel(str(tmp_path / "b.ibu"), str(tmp_path / "b.ibu.gz"), workers=1)
    _write(ia, tmp_path / "loose.ibu", loose, sorted_flag=False)
    ins = [tmp_path / "a.ibu", tmp_path / "b.ibu.gz", tmp_path / "c.ibu"]
    for extra, want in (([], _sort(np.concatenate(parts))), ([tmp_path / "loose.ibu", "--sort-unsorted"], _sort(np.concatenate(parts + [loose])))):
        out = tmp_path / f"out{len(extra)}.ibu"
        r = subprocess.run([str(exe), str(out), *[str(p) for p in ins + extra]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        h, got = ia.load_to_vec(str(out))
        assert h.sorted() and (h.bc_len, h.umi_len) == (16, 12)
        assert np.asarray(got).tobytes() == want.tobytes()
        assert np.asarray(got).tobytes() == mnp.merge_runs(np.concatenate(parts + ([_sort(loose)] if extra else [])), [len(p) for p in parts] + ([len(loose)] if extra else [])).tobytes()
