"""The count matrix on the device (ibu_records_swap_umi_index, ibu_pair_counts, ibu_count_matrix): every comparison is byte
for byte against the numpy statement of the semantics in tests/count_np.py, every call goes through the C ABI, and every
buffer is carved at exactly its contract size out of an arena with guard zones (the pattern of tests/test_gpu_guards.py)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import count_np as cnp
from tests import whitelist_np as wnp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 63, 127, 128, 129, 255, 2559, 2561, 5121, 100_003, 1_000_003]
SEG, TILE = 8192, 128                                            # k_aggregate.hip: records per segment / per tile
SEAMS = [SEG * k + d for k in (1, 2, 12) for d in (-1, 0, 1)] + [TILE * k + d for k in (3, 63, 65) for d in (-1, 0, 1)]
PAIR_NS = SIZES + SEAMS
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
SHAPES = ["few", "own_pair", "one_pair", "new_index", "seam"]
SWAP_GRID = list(itertools.product(SIZES, SKEWS, SKEWS))
PAIR_GRID = list(itertools.product(PAIR_NS, SKEWS, SHAPES))
MATRIX_GRID = list(itertools.product([1, 2, 129, 5121, 100_003, 1_000_003], [0, 1], SKEWS))
assert len(SIZES) == 13 and len(set(PAIR_NS)) == len(PAIR_NS) == 31, PAIR_NS
assert len(SWAP_GRID) == 52 and len(PAIR_GRID) == 310 and len(MATRIX_GRID) == 24
GUARD, PATTERN = 4096, 0xA5


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


class Arena:
    """One allocation, pattern-filled; carve(nbytes, skew) hands out a view that starts `skew` bytes behind a 256-byte
    boundary with at least GUARD pattern bytes on either side; check() looks at every byte outside the views."""

    def __init__(self, ia, ctx, total):
        self.ia, self.ctx = ia, ctx
        self.total = total
        self.buf = ctx.upload(np.full(total, PATTERN, np.uint8))
        self.pos = GUARD
        self.used = []

    def carve(self, nbytes, skew=0):
        start = (self.pos + 255) // 256 * 256 + skew
        assert start + nbytes + GUARD <= self.total, "arena too small"
        self.used.append((start, start + nbytes))
        self.pos = start + nbytes + GUARD
        return self.ia.DeviceBuffer.wrap(self.ctx, self.buf.ptr + start, max(nbytes, 1))

    def check(self, what):
        self.ctx.synchronize()
        host = self.buf.download(np.uint8)
        mask = np.ones(self.total, bool)
        for a, b in self.used:
            mask[a:b] = False
        bad = np.flatnonzero(mask & (host != PATTERN))
        assert bad.size == 0, f"{what}: {bad.size} guard bytes overwritten, first at arena offset {int(bad[0])} (views: {self.used})"

    def free(self):
        self.buf.free()


def _arena(ia, ctx, *sizes):
    return Arena(ia, ctx, sum(sizes) + (len(sizes) + 2) * (GUARD + 512) + 4096)


def _p(buf):
    return C.c_void_p(buf.ptr) if buf is not None else None


def _swap(ia, ctx, src, dst, n, stream=None):
    ia._check(ia.lib.ibu_records_swap_umi_index(ctx._c, _p(src), _p(dst), n, stream))


def _pair_counts(ia, ctx, d, n, outs, cap, stream=None):
    """-> (n_pairs, n_triples) of one ibu_pair_counts call; outs = four DeviceBuffers or None."""
    npairs, ntriples = C.c_size_t(12345), C.c_size_t(12345)
    ia._check(ia.lib.ibu_pair_counts(ctx._c, _p(d), n, *[_p(o) for o in outs], cap, C.byref(npairs), C.byref(ntriples), stream))
    return npairs.value, ntriples.value


def _count_matrix(ia, ctx, d, tmp, n, flags, outs, cap, stream=None):
    ne, nm = C.c_size_t(12345), C.c_size_t(12345)
    ia._check(ia.lib.ibu_count_matrix(ctx._c, _p(d), _p(tmp), n, flags, *[_p(o) for o in outs], cap, C.byref(ne), C.byref(nm), stream))
    return ne.value, nm.value


def _download(outs, k):
    return [o.download(np.uint64, k) if k else np.empty(0, np.uint64) for o in outs]


def _same(got, want):
    return all(g.tobytes() == np.ascontiguousarray(w, np.uint64).tobytes() for g, w in zip(got, want))


def _random_records(seed, n, n_barcodes=30, n_indices=10, n_umis=8, bc_len=16):
    return cnp.make_records(np.random.default_rng(seed), n, bc_len, n_barcodes, n_indices, n_umis)


# ---- the field exchange ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,skew_src,skew_dst", SWAP_GRID)
def test_swap_out_of_place(ia, ctx, n, skew_src, skew_dst):
    recs = _random_records(0xC0100 + n, n)
    ar = _arena(ia, ctx, 24 * n, 24 * n, 24 * n)
    try:
        src, dst, back = ar.carve(24 * n, skew_src), ar.carve(24 * n, skew_dst), ar.carve(24 * n, skew_src)
        if n:
            src.upload(recs)
        _swap(ia, ctx, src, dst, n)
        _swap(ia, ctx, dst, back, n)
        ar.check("swap out of place")
        if n:
            assert src.download(count=24 * n).tobytes() == recs.tobytes(), "the source is not written"
            assert dst.download(count=24 * n).tobytes() == cnp.swap(recs).tobytes()
            assert back.download(count=24 * n).tobytes() == recs.tobytes(), "twice is the identity"
    finally:
        ar.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("skew", SKEWS)
def test_swap_in_place(ia, ctx, n, skew):
    recs = _random_records(0xC0200 + n, n)
    ar = _arena(ia, ctx, 24 * n)
    try:
        d = ar.carve(24 * n, skew)
        if n:
            d.upload(recs)
        _swap(ia, ctx, d, d, n)
        ar.check("swap in place")
        if n:
            assert d.download(count=24 * n).tobytes() == cnp.swap(recs).tobytes()
        _swap(ia, ctx, d, d, n)
        ar.check("swap in place, again")
        if n:
            assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        ar.free()


def test_swap_refuses_partial_overlap_and_bad_pointers(ia, ctx):
    n = 1000
    recs = _random_records(0xC0300, n + 10)
    d = ctx.upload(recs)
    m = n - 5
    for shift in (24, -24, 24 * (m - 1), -24 * (m - 1), 8, -8, 128):   # both views stay inside the allocation
        a = ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * 5, 24 * m)
        b = ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * 5 + shift, 24 * m)
        if abs(shift) < 24 * m - 24 * 4:                          # (the far shifts would leave the allocation with m records)
            with pytest.raises(ia.IbuError) as ei:
                _swap(ia, ctx, a, b, m)
            assert ei.value.kind == "InvalidArg", shift
        k = abs(shift) // 24 + 1 if abs(shift) >= 24 else 1       # as many records as make the ranges overlap by at least one word
        if 0 < abs(shift) < 24 * 5:
            with pytest.raises(ia.IbuError) as ei:
                _swap(ia, ctx, a, b, k + 1)
            assert ei.value.kind == "InvalidArg", shift
    # ranges that only touch are fine
    a = ia.DeviceBuffer.wrap(ctx, d.ptr, 24 * 5)
    b = ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * 5, 24 * 5)
    _swap(ia, ctx, a, b, 5)
    ctx.synchronize()
    for bad in (ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 24), None):
        with pytest.raises(ia.IbuError) as ei:
            _swap(ia, ctx, a, bad, 1)
        assert ei.value.kind == "InvalidArg"
    with pytest.raises(ia.IbuError) as ei:
        _swap(ia, ctx, a, a, 1 << 40)
    assert ei.value.kind == "InvalidArg"
    ctx.synchronize()
    got = d.download(cnp.REC, n + 10)
    assert got[:5].tobytes() == recs[:5].tobytes() and got[5:10].tobytes() == cnp.swap(recs[:5]).tobytes()
    assert got[10:].tobytes() == recs[10:].tobytes(), "a refused call writes nothing"
    d.free()


# ---- pair_counts ----------------------------------------------------------------------------------------------------
def _shape(shape, n, skew):
    """Records in {w0, w1, w2} form and what the numpy side must find in them."""
    r = np.zeros(n, cnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.uint64)
    if shape == "few":                                           # few barcodes x few indices with duplicated UMIs, sorted
        r = cnp.count_matrix(_random_records(0xC0400 + n, n, n_barcodes=8, n_indices=5, n_umis=6))[1]
        e = cnp.pair_counts(r)
        assert len(e[0]) <= 40
        if n >= 5121:
            assert len(e[0]) == 40 and (e[3] < e[2]).all() and (e[3] > 1).all(), "every pair has several UMIs, each read more than once"
    elif shape == "own_pair":                                    # every record its own pair
        w[:, 0], w[:, 1], w[:, 2] = i >> np.uint64(1), i & np.uint64(1), 9
        assert len(cnp.pair_counts(r)[0]) == n
    elif shape == "one_pair":                                    # one pair for all n, a new third word every four records
        w[:, 0], w[:, 1], w[:, 2] = 5, 6, i >> np.uint64(2)
        e = cnp.pair_counts(r)
        assert len(e[0]) == min(n, 1) and (n == 0 or (int(e[2][0]), int(e[3][0])) == (n, (n + 3) // 4))
    elif shape == "new_index":                                   # one barcode, every record a new index
        w[:, 0], w[:, 1], w[:, 2] = 7, i, 3
        e = cnp.pair_counts(r)
        assert len(e[0]) == n and len(np.unique(w[:, 0])) == min(n, 1)
    else:                                                        # runs that begin on the last record of a segment and on the first of the next
        head = min(skew // 8, n)                                 # an 8- but not 16-byte aligned base peels one record in front of segment 1
        heads = np.zeros(n, bool)
        heads[:1] = True
        for j in range(1, n // SEG + 2):
            for row in (SEG * j - 1 + head, SEG * j + head):
                if row < n:
                    heads[row] = True
        w[:, 0], w[:, 1], w[:, 2] = np.cumsum(heads), 1, i // np.uint64(3)
        e = cnp.pair_counts(r)
        starts = np.concatenate([[0], np.cumsum(e[2])[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
        assert starts.tolist() == np.flatnonzero(heads).tolist()
        for j in range(1, (n - head) // SEG + 1):
            if SEG * j + head < n:
                assert heads[SEG * j - 1 + head] and heads[SEG * j + head], "a head on either side of the seam"
    return r


@pytest.mark.parametrize("n,skew,shape", PAIR_GRID)
def test_pair_counts_matches_numpy(ia, ctx, n, skew, shape):
    recs = _shape(shape, n, skew)
    want = cnp.pair_counts(recs)
    k = len(want[0])
    ar = _arena(ia, ctx, 24 * n, *[8 * k] * 4)
    try:
        d = ar.carve(24 * n, skew)
        if n:
            d.upload(recs)
        outs = [ar.carve(8 * k, s) for s in (skew, 0, 8, skew)]
        assert _pair_counts(ia, ctx, d, n, [None] * 4, 0) == (k, int(want[3].sum())), "size query"
        ar.check("pair_counts size query")
        if k:
            assert all((o.download(np.uint8, 8 * k) == PATTERN).all() for o in outs), "a size query writes nothing"
        assert _pair_counts(ia, ctx, d, n, outs, k) == (k, int(want[3].sum())), "cap exact"
        ar.check(f"pair_counts {shape}")
        assert _same(_download(outs, k), want)
        assert n == 0 or d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
    finally:
        ar.free()


def test_pair_counts_full_64_bit_words(ia, ctx):
    """32-base barcodes: 0 and all ones are legal codes, and all three words use all 64 bits."""
    rng = np.random.default_rng(0xC0500)
    n = 50_000
    vals = np.concatenate([np.array([0, 2**64 - 1, 1 << 63, (1 << 63) - 1], np.uint64), rng.integers(0, 2**64, 6, dtype=np.uint64, endpoint=False)])
    r = np.zeros(n, cnp.REC)
    for f in ("barcode", "umi", "index"):
        r[f] = vals[rng.integers(0, len(vals), n)]
    (want, s) = cnp.count_matrix(r)
    assert 0 in want[0] and 2**64 - 1 in want[0] and 2**64 - 1 in want[1] and (want[2] > want[3]).any()
    d = ctx.upload(s)
    got = ctx.pair_counts(d, n)
    assert _same(got, want)
    d.free()


def test_pair_counts_on_unsorted_input_is_the_run_length_encoding(ia, ctx):
    n = 300_001
    r = _random_records(0xC0600, n, n_barcodes=3, n_indices=2, n_umis=2)
    want = cnp.pair_counts(r)
    assert len(want[0]) > n // 10 and len(want[0]) > len(cnp.count_matrix(r)[0][0]), "far more runs than distinct pairs"
    assert (want[3] > 1).any() and (want[2] > want[3]).any()
    d = ctx.upload(r)
    assert _same(ctx.pair_counts(d, n), want)
    # the molecule view of ordinarily sorted records: (barcode, umi) with their reads and distinct indices
    s = cnp.sort_records(r)
    d.upload(s)
    mol = ctx.pair_counts(d, n)
    assert _same(mol, cnp.pair_counts(s)) and (mol[3] >= 2).any(), "a (barcode, umi) seen with two indices"
    d.free()


def test_pair_counts_forms_of_the_call(ia, ctx):
    n = 100_003
    s = cnp.count_matrix(_random_records(0xC0700, n, n_barcodes=300, n_indices=40))[1]
    want = cnp.pair_counts(s)
    k, triples = len(want[0]), int(want[3].sum())
    ar = _arena(ia, ctx, 24 * n, *[8 * k] * 4)
    try:
        d = ar.carve(24 * n, 8)
        d.upload(s)
        outs = [ar.carve(8 * k, 0) for _ in range(4)]
        # cap one too small: the error carries the count, nothing is written
        npairs, ntriples = C.c_size_t(), C.c_size_t()
        rc = ia.lib.ibu_pair_counts(ctx._c, _p(d), n, *[_p(o) for o in outs], k - 1, C.byref(npairs), C.byref(ntriples), None)
        with pytest.raises(ia.IbuError) as ei:
            ia._check(rc)
        assert ei.value.kind == "InvalidArg" and (ei.value.a, ei.value.b) == (k, k - 1)
        assert (npairs.value, ntriples.value) == (k, triples)
        ar.check("pair_counts, cap one too small")
        assert all((o.download(np.uint8, 8 * k) == PATTERN).all() for o in outs), "nothing written"
        # no distinct_third: the other three are written, *n_triples is still reported
        assert _pair_counts(ia, ctx, d, n, outs[:3] + [None], k) == (k, triples)
        ar.check("pair_counts without distinct_third")
        assert _same(_download(outs[:3], k), want[:3]) and (outs[3].download(np.uint8, 8 * k) == PATTERN).all()
        # n_triples is nullable
        ia._check(ia.lib.ibu_pair_counts(ctx._c, _p(d), n, *[_p(o) for o in outs], k + 7, C.byref(npairs), None, None))
        ar.check("pair_counts, larger cap")
        assert npairs.value == k and _same(_download(outs, k), want)
        # argument errors
        for args in ((ia.DeviceBuffer.wrap(ctx, d.ptr + 4, 24), 1, outs, 1), (None, 1, outs, 1), (d, 1 << 40, outs, 1), (d, n, [outs[0], None, outs[2], outs[3]], k),
                     (d, n, [ia.DeviceBuffer.wrap(ctx, outs[0].ptr + 4, 8)] + outs[1:], k)):
            with pytest.raises(ia.IbuError) as ei:
                _pair_counts(ia, ctx, *args)
            assert ei.value.kind == "InvalidArg"
        with pytest.raises(ia.IbuError) as ei:
            ia._check(ia.lib.ibu_pair_counts(ctx._c, _p(d), n, None, None, None, None, 0, None, None, None))
        assert ei.value.kind == "InvalidArg"
        assert _pair_counts(ia, ctx, None, 0, [None] * 4, 0) == (0, 0)
    finally:
        ar.free()


def test_pair_counts_on_two_streams_of_two_contexts(ia, ctx):
    n = 1_000_003
    ra, rb = (cnp.count_matrix(_random_records(0xC0800 + j, n, n_barcodes=1000, n_indices=50))[1] for j in (0, 1))
    wa, wb = cnp.pair_counts(ra), cnp.pair_counts(rb)
    other = ia.Context(0)                                        # its stream is a second hardware queue on the same device
    try:
        da, db = ctx.upload(ra), other.upload(rb)
        oa, ob = [ctx.alloc(8 * len(wa[0])) for _ in range(4)], [other.alloc(8 * len(wb[0])) for _ in range(4)]
        for _ in range(3):
            assert _pair_counts(ia, ctx, da, n, oa, len(wa[0]))[0] == len(wa[0])
            assert _pair_counts(ia, other, db, n, ob, len(wb[0]), stream=other.stream)[0] == len(wb[0])
        ctx.synchronize()
        other.synchronize(other.stream)
        assert _same(_download(oa, len(wa[0])), wa) and _same(_download(ob, len(wb[0])), wb)
        for b in [da, db] + oa + ob:
            b.free()
    finally:
        other.close()


def test_barcode_counts_on_swapped_sorted_records_gives_the_csr_row_lengths(ia, ctx):
    n = 200_003
    r = _random_records(0xC0900, n, n_barcodes=500, n_indices=30, n_umis=20)
    (b, i, reads, umis), s = cnp.count_matrix(r)
    d = ctx.upload(s)
    got_b, got_reads, got_rows = ctx.barcode_counts(d, n)
    ub, inv = np.unique(b, return_inverse=True)
    assert (got_b == ub).all() and (got_rows == np.bincount(inv).astype(np.uint64)).all()
    assert (got_reads == np.bincount(inv, weights=reads.astype(np.float64)).astype(np.uint64)).all()
    assert int(got_rows.sum()) == len(b)
    d.free()


# ---- count_matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,flags,skew", MATRIX_GRID)
def test_count_matrix_matches_numpy(ia, ctx, n, flags, skew):
    r = _random_records(0xC0A00 + n, n, n_barcodes=200, n_indices=25, n_umis=12)
    assert n < 3 or not (np.diff(r["barcode"].astype(np.float64)) >= 0).all(), "the input is not sorted"
    want, s = cnp.count_matrix(r)
    k = len(want[0])
    ar = _arena(ia, ctx, 24 * n, 24 * n, *[8 * k] * 4)
    try:
        d, tmp = ar.carve(24 * n, skew), ar.carve(24 * n, skew)
        d.upload(r)
        outs = [ar.carve(8 * k, 0) for _ in range(4)]
        assert _count_matrix(ia, ctx, d, tmp, n, flags, outs, k) == (k, int(want[3].sum()))
        ar.check("count_matrix")
        assert _same(_download(outs, k), want)
        after = s if flags else cnp.swap(s)
        assert d.download(count=24 * n).tobytes() == after.tobytes()
    finally:
        ar.free()


def test_count_matrix_forms_of_the_call(ia, ctx):
    n = 50_001
    r = _random_records(0xC0B00, n, n_barcodes=100, n_indices=10)
    want, s = cnp.count_matrix(r)
    k = len(want[0])
    ar = _arena(ia, ctx, 24 * n, 24 * n, *[8 * k] * 4)
    try:
        d, tmp = ar.carve(24 * n, 0), ar.carve(24 * n, 0)
        outs = [ar.carve(8 * k, 0) for _ in range(4)]
        d.upload(r)
        for flags in (2, 3, 1 << 31):                            # an unknown bit: refused before anything is touched
            with pytest.raises(ia.IbuError) as ei:
                _count_matrix(ia, ctx, d, tmp, n, flags, outs, k)
            assert ei.value.kind == "InvalidArg"
        assert d.download(count=24 * n).tobytes() == r.tobytes()
        for flags in (0, ia.COUNT_LEAVE_SWAPPED):                # cap too small: after the sort, with the records as the flags promise
            d.upload(r)
            ne, nm = C.c_size_t(), C.c_size_t()
            rc = ia.lib.ibu_count_matrix(ctx._c, _p(d), _p(tmp), n, flags, *[_p(o) for o in outs], k - 1, C.byref(ne), C.byref(nm), None)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(rc)
            assert ei.value.kind == "InvalidArg" and (ei.value.a, ei.value.b) == (k, k - 1) and ne.value == k
            ar.check("count_matrix, cap one too small")
            assert all((o.download(np.uint8, 8 * k) == PATTERN).all() for o in outs)
            assert d.download(count=24 * n).tobytes() == (s if flags else cnp.swap(s)).tobytes()
        d.upload(r)                                              # no umis column, no molecule total
        ne = C.c_size_t()
        ia._check(ia.lib.ibu_count_matrix(ctx._c, _p(d), _p(tmp), n, 0, _p(outs[0]), _p(outs[1]), _p(outs[2]), None, k, C.byref(ne), None, None))
        ar.check("count_matrix without umis")
        assert ne.value == k and _same(_download(outs[:3], k), want[:3])
        with pytest.raises(ia.IbuError) as ei:                   # no size query
            _count_matrix(ia, ctx, d, tmp, n, 0, [None] * 4, 0)
        assert ei.value.kind == "InvalidArg"
        assert _count_matrix(ia, ctx, None, None, 0, 0, [None] * 4, 0) == (0, 0)
        # the Python wrapper
        d.upload(r)
        assert _same(ctx.count_matrix(d, tmp, n), want)
        d.upload(r)
        assert _same(ctx.count_matrix(d, tmp, n, cap=k, leave_swapped=True), want)
    finally:
        ar.free()


def _noisy_case(n, w, bc_len, seed, n_features=50):
    rng = np.random.default_rng(seed)
    wl, bc = wnp.make_case(rng, bc_len, w, n, junk=False, shares=(0.94, 0.05, 0.0, 0.01))
    recs = np.zeros(n, cnp.REC)
    recs["barcode"] = bc
    recs["umi"] = rng.integers(0, 64, n, dtype=np.uint64)
    recs["index"] = rng.integers(0, n_features, n, dtype=np.uint64)
    return wl, recs


def _numpy_chain(recs, wl, bc_len):
    want, cls, counts = wnp.correct_records(recs, wl, bc_len, 1)
    return cnp.count_matrix(want[np.isin(cls, (0, 1))])[0], counts


def test_correct_select_count_matrix_end_to_end(ia, ctx):
    n, w, bc_len = 1_000_000, 2000, 16
    wl, recs = _noisy_case(n, w, bc_len, 0xC0C00)
    want, counts = _numpy_chain(recs, wl, bc_len)
    assert len(np.unique(want[0])) <= w and (want[3] < want[2]).any() and len(want[0]) <= w * 50
    d = ctx.upload(recs)
    codes = ctx.upload(wl)
    with ia.Whitelist(ctx, codes, len(wl), bc_len) as h:
        d_cls = ctx.alloc(n)
        assert ctx.correct_barcodes(h, d, n, 1, d_cls) == counts
    out, k = ctx.select_records(d, d_cls, n, 0b0011)
    assert k == counts["exact"] + counts["corrected"]
    got = ctx.count_matrix(out, d, k, cap=w * 50)                # the caller's bound: whitelist size x features
    assert _same(got, want)
    for b in (d, codes, d_cls, out):
        b.free()


def test_count_file_example(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    n, w, bc_len = 50_000, 300, 16
    wl, recs = _noisy_case(n, w, bc_len, 0xC0D00, n_features=20)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    text = lambda c: "".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(bc_len))   # base i at bits [2i, 2i+1]
    (tmp_path / "wl.txt").write_text("\n".join(text(c) for c in wl) + "\n")
    for args, want in (((str(tmp_path / "wl.txt"),), _numpy_chain(recs, wl, bc_len)[0]), ((), cnp.count_matrix(recs)[0])):
        r = subprocess.run([str(exe), str(tmp_path / "in.ibu"), *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        matrix = [l for l in lines if not l.startswith("#")]
        assert matrix == [f"{text(b)}\t{int(i)}\t{int(u)}\t{int(c)}" for b, i, c, u in zip(*want)]
        ub, inv = np.unique(want[0], return_inverse=True)
        rows = [l for l in lines if l.startswith("#row\t")]
        reads = np.bincount(inv, weights=want[2].astype(np.float64)).astype(np.int64)
        assert rows == [f"#row\t{text(b)}\t{int(e)}\t{int(c)}" for b, e, c in zip(ub, np.bincount(inv), reads)]


def test_full_size_count_matrix_properties_1e9(ia, ctx):
    """1e9 records at once, through size-independent properties.  The records are the device generator's: 5e8 records of 8-base
    barcodes (65 536 of them) and 5-base UMIs (1024 values) with index = i, written twice, and passed through the field exchange —
    so the word in the index place has 1024 values, the word in the UMI place is i, and every molecule has exactly two reads: at most
    65 536 x 1024 = 6.7e7 entries under cap = 1e8.  (The library has no device-side modulo that would fold a generated stream to
    exactly 1e5 barcodes x 1000 indices; the generator's masks give the nearest powers of four.)"""
    n, half, cap = 1_000_000_000, 500_000_000, 100_000_000
    recs, tmp = ctx.alloc(24 * n), ctx.alloc(24 * n)
    outs = [ctx.alloc(8 * cap) for _ in range(4)]
    for lo in (0, half):
        ctx.generate(0xC0E00, 0, half, 8, 5, ia.DeviceBuffer.wrap(ctx, recs.ptr + 24 * lo, 24 * half))
    _swap(ia, ctx, recs, recs, n)                                # {barcode, i, umi5}: the 1024-valued word sits in the index place
    before = ctx.reduce(recs, n)
    assert before["count"] == n and before["sum"][1] == (2 * (half * (half - 1) // 2)) % 2**64
    assert not ctx.is_sorted(recs, n)
    ne, nm = _count_matrix(ia, ctx, recs, tmp, n, ia.COUNT_LEAVE_SWAPPED, outs, cap)
    assert ne <= 65_536 * 1024 and ne > 60_000_000 and nm == half, (ne, nm)
    # the records are the input multiset with the second and third words exchanged, in order
    after = ctx.reduce(recs, n)
    assert after["count"] == n
    assert after["sum"] == [before["sum"][0], before["sum"][2], before["sum"][1]]
    assert after["xor"] == [before["xor"][0], before["xor"][2], before["xor"][1]]
    assert ctx.is_sorted(recs, n)
    # ... so its first two words are barcode and index, and the pair total ibu_barcode_counts reports is the number of entries
    nb, npairs = C.c_size_t(), C.c_size_t()
    ia._check(ia.lib.ibu_barcode_counts(ctx._c, _p(recs), n, None, None, None, 0, C.byref(nb), C.byref(npairs), None))
    assert nb.value == 65_536 and npairs.value == ne
    b, i, reads, umis = _download(outs, ne)
    assert int(reads.sum()) == n and int(umis.sum()) == nm
    assert (reads == 2 * umis).all(), "every molecule was written twice"
    assert (b < 65_536).all() and (i < 1024).all()
    at = np.random.default_rng(0xC0E01).integers(0, ne - 1, 1_000_000)
    assert ((b[at] < b[at + 1]) | ((b[at] == b[at + 1]) & (i[at] < i[at + 1]))).all(), "entries strictly ascending by (barcode, index)"
    for buf in [recs, tmp] + outs:
        buf.free()
