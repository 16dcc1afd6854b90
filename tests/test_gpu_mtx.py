"""The matrix export on the device (ibu_matrix_rows, ibu_matrix_market_body): every comparison is byte for byte against the numpy /
Python statement of the semantics in tests/mtx_np.py; every call goes through the C ABI, and every buffer — the columns at exactly
8 B per entry, row_keys at exactly 8 B per row, row_ptr at 8 B per row and one more, the text at exactly its length and at odd byte
addresses — is carved at its contract size out of the guard-zone arena of tests/test_gpu_count.py.  The input columns are compared
after every case: they are never written.  One test per size, its shapes inside it: a case is milliseconds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import count_np as cnp
from tests import mtx_np
from tests.test_gpu_count import PATTERN, ROOT, _arena, _p

pytestmark = pytest.mark.gpu

UNIT = 2048                                                      # k_matrix.hip: entries per unit
SIZES = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 3 * UNIT - 1, 3 * UNIT + 1, 16 * UNIT + 1, 100_003]
BIG = 1024 * 16 * UNIT + 1                                       # one entry more than one iteration of the scan's outer loop takes
GARBAGE = 0x5A5A5A5A5A5A5A5A
TOP = (1 << 64) - 1
TEXT_SKEWS = [0, 1, 2, 3, 8]                                     # bytes from a 16-byte boundary
# 0, 10^k - 1 and 10^k for every k in 1 .. 19, 2^32 - 1, 2^32, 2^63, 2^64 - 1
BOUNDARIES = [0] + [v for k in range(1, 20) for v in (10 ** k - 1, 10 ** k)] + [(1 << 32) - 1, 1 << 32, 1 << 63, TOP]


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _rows(ia, ctx, d_first, n, outs, cap, stream=None):
    """One ibu_matrix_rows call through the C ABI -> *n_rows; outs = (row_of_entry, row_keys, row_ptr), DeviceBuffers or None."""
    nr = C.c_size_t(12345)
    ia._check(ia.lib.ibu_matrix_rows(ctx._c, _p(d_first), n, *[_p(o) for o in outs], cap, C.byref(nr), stream))
    return nr.value


def _body(ia, ctx, cols, n, add, d_text, cap, want_maxima=True, stream=None):
    """One ibu_matrix_market_body call through the C ABI -> (*n_bytes, maxima or None)."""
    nb = C.c_size_t(12345)
    mx = (C.c_uint64 * 3)(*[GARBAGE] * 3) if want_maxima else None
    ia._check(ia.lib.ibu_matrix_market_body(ctx._c, *[_p(c) for c in cols], n, add[0], add[1], _p(d_text), cap, C.byref(nb), mx, stream))
    return nb.value, (tuple(int(x) for x in mx) if want_maxima else None)


def _dl(buf, words):
    return buf.download(np.uint64, words) if words else np.empty(0, np.uint64)


# ---- rows ------------------------------------------------------------------------------------------------------------
ROW_SHAPES = ["one_row", "own_row", "rows_2047", "rows_2048", "rows_2049", "seam_head", "repeats", "random"]


def _row_shape(shape, n, seed=0):
    i = np.arange(n, dtype=np.uint64)
    if shape == "one_row":
        return np.full(n, 1 << 63, np.uint64)
    if shape == "own_row":
        return i * np.uint64(0x9E3779B97F4A7C15)                 # odd multiplier: a bijection, every entry its own row, 64-bit values
    if shape.startswith("rows_"):                                # heads at, before and after the unit seams
        return i // np.uint64(int(shape[5:]))
    if shape == "seam_head":                                     # the only head beside entry 0 is the first entry of the last unit
        return (i >= np.uint64(max((n - 1) // UNIT * UNIT, 1))).astype(np.uint64)
    if shape == "repeats":                                       # A A A B B B A A A ...: equal keys in runs that are not adjacent
        return (i // np.uint64(3)) % np.uint64(2) + np.uint64(7)
    rng = np.random.default_rng(0x3A7300 + n + seed)             # random run lengths: 1 .. 8, or (seed 1) 1 .. 1999
    top = 9 if seed == 0 else 2000
    lens = rng.integers(1, top, 3 * n // top + 16)
    ends = np.cumsum(lens)
    assert ends[-1] >= n
    k = int(np.searchsorted(ends, n)) + 1                        # the runs that begin in front of entry n, the last one cut there
    lens = lens[:k].copy()
    lens[-1] -= ends[k - 1] - n
    first = np.repeat(rng.integers(0, 5, k).astype(np.uint64) << np.uint64(61), lens)
    assert len(first) == n
    return first


def _check_rows(ia, ctx, first, label):
    n = len(first)
    want = mtx_np.matrix_rows(first)
    r = len(want[1])
    ar = _arena(ia, ctx, 8 * n, 8 * n, 8 * r, 8 * (r + 1))
    try:
        d = ar.carve(8 * n, 8)
        if n:
            d.upload(first)
        outs = [ar.carve(8 * n, 0), ar.carve(8 * r, 8), ar.carve(8 * (r + 1), 0)]
        assert _rows(ia, ctx, None if n == 0 else d, n, [None] * 3, 0) == r, label                 # the size query
        assert _rows(ia, ctx, None if n == 0 else d, n, outs, r) == r, label                       # cap == n_rows exactly
        ar.check(label)
        got = [_dl(outs[0], n), _dl(outs[1], r), _dl(outs[2], r + 1 if n else 0)]
        exp = [want[0], want[1], want[2] if n else want[2][:0]]                                  # no entries: nothing is touched
        for name, g, w in zip(("row_of_entry", "row_keys", "row_ptr"), got, exp):
            assert g.tobytes() == w.tobytes(), (label, name, np.flatnonzero(g != w)[:5])
        assert _dl(d, n).tobytes() == first.tobytes(), label
        if n == 0:
            assert (outs[2].download(np.uint8, 8) == PATTERN).all()
    finally:
        ar.free()


@pytest.mark.parametrize("n", SIZES)
def test_matrix_rows_matches_numpy(ia, ctx, n):
    for shape in ROW_SHAPES:
        first = _row_shape(shape, n)
        if n > UNIT and shape == "seam_head":
            assert np.flatnonzero(np.diff(first)).tolist() == [(n - 1) // UNIT * UNIT - 1]
        _check_rows(ia, ctx, first, f"n={n} {shape}")


def test_matrix_rows_second_iteration_of_the_scan(ia, ctx):
    first = _row_shape("random", BIG, seed=1)                    # long runs: tens of thousands of rows
    assert len(first) == BIG and BIG > 1024 * 16 * UNIT
    _check_rows(ia, ctx, first, f"n={BIG} random")


def test_matrix_rows_forms_of_the_call(ia, ctx):
    n = 3 * UNIT + 77
    first = _row_shape("random", n)
    want = mtx_np.matrix_rows(first)
    r = len(want[1])
    sizes = (8 * n, 8 * r, 8 * (r + 1))
    ar = _arena(ia, ctx, 8 * n, *sizes, *sizes, *sizes)
    try:
        d = ar.carve(8 * n, 0)
        d.upload(first)
        for k in range(3):                                       # each output alone
            out = ar.carve(sizes[k], 0)
            assert _rows(ia, ctx, d, n, [out if j == k else None for j in range(3)], r) == r
            ar.check(f"output {k} alone")
            assert _dl(out, sizes[k] // 8).tobytes() == want[k].tobytes(), k
        outs = [ar.carve(s, 0) for s in sizes]
        nr = C.c_size_t(12345)                                   # cap one too small: refused, *n_rows set, nothing written
        rc = ia.lib.ibu_matrix_rows(ctx._c, _p(d), n, *[_p(o) for o in outs], r - 1, C.byref(nr), None)
        with pytest.raises(ia.IbuError) as ei:
            ia._check(rc)
        assert ei.value.kind == "InvalidArg" and (ei.value.a, ei.value.b) == (r, r - 1) and nr.value == r
        ar.check("cap one too small")
        assert all((o.download(np.uint8, s) == PATTERN).all() for o, s in zip(outs, sizes))
        assert _rows(ia, ctx, d, n, [None] * 3, 5) == r           # nothing asked for: the count, whatever cap says
        for bad in ([C.c_void_p(outs[0].ptr + 4), outs[1], outs[2]], [outs[0], outs[1], C.c_void_p(outs[2].ptr + 1)]):
            with pytest.raises(ia.IbuError) as ei:                # a misaligned output
                ia._check(ia.lib.ibu_matrix_rows(ctx._c, _p(d), n, *[b if isinstance(b, C.c_void_p) else _p(b) for b in bad], r, C.byref(nr), None))
            assert ei.value.kind == "InvalidArg"
        for args in ((None, n), (C.c_void_p(d.ptr + 4), n), (_p(d), 1 << 40)):   # NULL / misaligned column, too many entries
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_matrix_rows(ctx._c, args[0], args[1], *[_p(o) for o in outs], r, C.byref(nr), None))
            assert ei.value.kind == "InvalidArg"
        with pytest.raises(ia.IbuError):
            ia._check(ia.lib.ibu_matrix_rows(ctx._c, _p(d), n, None, None, None, 0, None, None))   # n_rows is NULL
        ar.check("refused calls")
        assert all((o.download(np.uint8, s) == PATTERN).all() for o, s in zip(outs, sizes))
        assert _dl(d, n).tobytes() == first.tobytes()
        # the Python wrapper
        rows = ctx.matrix_rows(d, n)
        assert rows.n_rows == r
        assert [_dl(rows.d_row_of_entry, n).tobytes(), _dl(rows.d_keys, r).tobytes(), _dl(rows.d_ptr, r + 1).tobytes()] == [w.tobytes() for w in want]
        rows = ctx.matrix_rows(d, n, ordinals=False)
        assert rows.d_row_of_entry is None and _dl(rows.d_ptr, r + 1).tobytes() == want[2].tobytes()
        empty = ctx.matrix_rows(None, 0)
        assert empty.n_rows == 0 and _dl(empty.d_ptr, 1).tolist() == [0]
    finally:
        ar.free()


# ---- body ------------------------------------------------------------------------------------------------------------
BODY_SHAPES = ["zeros", "full", "alternate", "digits", "boundaries"]


def _digits_uniform(rng, n):
    """Values whose digit count is uniform on 1 .. 20."""
    d = rng.integers(1, 21, n)
    lo = np.array([0] + [10 ** k for k in range(1, 20)], dtype=object)[d - 1]
    hi = np.array([10 ** k for k in range(1, 20)] + [1 << 64], dtype=object)[d - 1]
    u = rng.integers(0, 1 << 63, n).astype(object) * 2 + rng.integers(0, 2, n).astype(object)
    return np.array([int(l + x % (h - l)) for l, h, x in zip(lo, hi, u)], dtype=np.uint64) if n else np.empty(0, np.uint64)


def _body_shape(shape, n):
    i = np.arange(n)
    if shape == "zeros":                                         # with no addend every line is "0 0 0\n": 6 bytes
        return [np.zeros(n, np.uint64)] * 3
    if shape == "full":                                          # ... every line 63 bytes; with an addend of 1 the first two print 0
        return [np.full(n, TOP, np.uint64)] * 3
    if shape == "alternate":
        return [np.where(i % 2 == 0, np.uint64(0), np.uint64(TOP))] * 3
    if shape == "digits":
        rng = np.random.default_rng(0x3A7400 + n)
        return [_digits_uniform(rng, n) for _ in range(3)]
    b = np.array(BOUNDARIES, np.uint64)                          # every boundary value in every column
    return [b[(i + shift) % len(b)] for shift in (0, 7, 13)]


def _check_body(ia, ctx, cols, add, skew, label, col_skew=0):
    n = len(cols[0])
    want, want_max = mtx_np.body(*[c.tolist() for c in cols], *add)
    nbytes = len(want)
    ar = _arena(ia, ctx, 8 * n, 8 * n, 8 * n, nbytes)
    try:
        d_cols = [ar.carve(8 * n, col_skew) for _ in range(3)]
        for d, c in zip(d_cols, cols):
            if n:
                d.upload(c)
        d_text = ar.carve(nbytes, skew)
        given = [None] * 3 if n == 0 else d_cols
        assert _body(ia, ctx, given, n, add, None, 0) == (nbytes, want_max), label                # the size query
        assert _body(ia, ctx, given, n, add, d_text, nbytes) == (nbytes, want_max), label         # cap_bytes exact
        ar.check(label)                                          # the bytes in front of the text and behind it included
        got = d_text.download(np.uint8, nbytes).tobytes() if nbytes else b""
        if got != want:
            at = next(k for k in range(nbytes) if got[k] != want[k])
            raise AssertionError(f"{label}: text differs at byte {at} of {nbytes}: {got[max(at - 30, 0):at + 30]!r} / {want[max(at - 30, 0):at + 30]!r}")
        for d, c in zip(d_cols, cols):
            assert _dl(d, n).tobytes() == c.tobytes(), label
    finally:
        ar.free()


@pytest.mark.parametrize("n", SIZES)
def test_matrix_market_body_matches_python(ia, ctx, n):
    k = 0
    for shape in BODY_SHAPES:
        cols = _body_shape(shape, n)
        for add in ((0, 0), (1, 1)):                             # "full" with (1, 1) is the wrap: 2^64 - 1 prints 0
            _check_body(ia, ctx, cols, add, TEXT_SKEWS[k % len(TEXT_SKEWS)], f"n={n} {shape} add={add}", col_skew=8 * (k & 1))
            k += 1


@pytest.mark.parametrize("skew", TEXT_SKEWS)
def test_matrix_market_body_text_at_any_byte_alignment(ia, ctx, skew):
    for n in (1, 65, 3 * UNIT + 1):
        for shape in ("digits", "alternate"):
            _check_body(ia, ctx, _body_shape(shape, n), (1, TOP), skew, f"n={n} {shape} skew={skew}")


def test_matrix_market_body_second_iteration_of_the_scan(ia, ctx):
    """One periodic column given three times (the columns are never written, so they may be one array): a pattern of seven lines
    repeated, whose text is a short byte string multiplied."""
    pattern = [0, 5, 9, 10, 99, 100, (1 << 32) - 1]
    block, block_max = mtx_np.body(pattern, pattern, pattern, 1, 0)
    reps, rest = divmod(BIG, len(pattern))
    want = block * reps + mtx_np.body(pattern[:rest], pattern[:rest], pattern[:rest], 1, 0)[0]
    col = np.tile(np.array(pattern, np.uint64), reps + 1)[:BIG]
    ar = _arena(ia, ctx, 8 * BIG, len(want))
    try:
        d = ar.carve(8 * BIG, 0)
        d.upload(col)
        d_text = ar.carve(len(want), 1)
        assert _body(ia, ctx, [d, d, d], BIG, (1, 0), d_text, len(want)) == (len(want), block_max)
        ar.check("periodic body")
        got = d_text.download(np.uint8, len(want))
        bad = np.flatnonzero(got != np.frombuffer(want, np.uint8))
        assert bad.size == 0, (bad[:5], bytes(got[bad[0] - 20:bad[0] + 20]), want[bad[0] - 20:bad[0] + 20])
        del got, bad
        assert _dl(d, BIG).tobytes() == col.tobytes()
    finally:
        ar.free()


def test_matrix_market_body_forms_of_the_call(ia, ctx):
    n = UNIT + 301
    cols = _body_shape("digits", n)
    want, want_max = mtx_np.body(*[c.tolist() for c in cols], 1, 1)
    nbytes = len(want)
    ar = _arena(ia, ctx, 8 * n, 8 * n, 8 * n, nbytes, nbytes)
    try:
        d_cols = [ar.carve(8 * n, 0) for _ in range(3)]
        for d, c in zip(d_cols, cols):
            d.upload(c)
        d_text = ar.carve(nbytes, 3)
        nb, mx = C.c_size_t(12345), (C.c_uint64 * 3)(*[GARBAGE] * 3)   # one byte too few: refused, *n_bytes and maxima set, nothing written
        rc = ia.lib.ibu_matrix_market_body(ctx._c, *[_p(c) for c in d_cols], n, 1, 1, _p(d_text), nbytes - 1, C.byref(nb), mx, None)
        with pytest.raises(ia.IbuError) as ei:
            ia._check(rc)
        assert ei.value.kind == "InvalidArg" and (ei.value.a, ei.value.b) == (nbytes, nbytes - 1) and nb.value == nbytes
        assert tuple(int(x) for x in mx) == want_max
        ar.check("cap_bytes one too small")
        assert (d_text.download(np.uint8, nbytes) == PATTERN).all()
        assert _body(ia, ctx, d_cols, n, (1, 1), d_text, nbytes, want_maxima=False) == (nbytes, None)   # maxima NULL
        assert d_text.download(np.uint8, nbytes).tobytes() == want
        d_more = ar.carve(nbytes, 2)                             # more room than needed: the bytes behind the text stay
        short = mtx_np.body(*[c.tolist() for c in cols], 0, 0)[0]
        assert len(short) < nbytes and _body(ia, ctx, d_cols, n, (0, 0), d_more, nbytes)[0] == len(short)
        got = d_more.download(np.uint8, nbytes)
        assert got[:len(short)].tobytes() == short and (got[len(short):] == PATTERN).all()
        ar.check("calls that write")
        before = d_text.download(np.uint8, nbytes).tobytes()
        refused = [([None, d_cols[1], d_cols[2]], n, _p(d_text), nbytes),                         # a NULL column
                   ([C.c_void_p(d_cols[0].ptr + 4), d_cols[1], d_cols[2]], n, _p(d_text), nbytes),  # a misaligned column
                   (d_cols, 1 << 40, _p(d_text), nbytes),                                          # too many entries
                   (d_cols, n, None, nbytes),                                                      # no text, and no size query either
                   (d_cols, n, C.c_void_p(d_cols[1].ptr + 8 * n - 1), nbytes)]                     # the text would overlap a column
        for given, count, text, cap in refused:
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_matrix_market_body(ctx._c, *[g if isinstance(g, C.c_void_p) or g is None else _p(g) for g in given], count, 1, 1,
                                                        text, cap, C.byref(nb), None, None))
            assert ei.value.kind == "InvalidArg"
        with pytest.raises(ia.IbuError):
            ia._check(ia.lib.ibu_matrix_market_body(ctx._c, *[_p(c) for c in d_cols], n, 1, 1, None, 0, None, None, None))   # n_bytes is NULL
        ar.check("refused calls")
        assert d_text.download(np.uint8, nbytes).tobytes() == before
        for d, c in zip(d_cols, cols):
            assert _dl(d, n).tobytes() == c.tobytes()
        assert _body(ia, ctx, [None] * 3, 0, (1, 1), d_text, nbytes) == (0, (0, 0, 0))               # no entries: nothing touched
        assert d_text.download(np.uint8, nbytes).tobytes() == before
        # the Python wrapper
        d_out, k, maxima = ctx.matrix_market_body(*d_cols, n)
        assert (k, maxima) == (nbytes, want_max) and d_out.download(np.uint8, k).tobytes() == want
    finally:
        ar.free()


# ---- end to end --------------------------------------------------------------------------------------------------------
BC_LEN, N_FEATURES = 16, 30


def _text(code, bc_len=BC_LEN):
    return "".join("ACGT"[(int(code) >> (2 * i)) & 3] for i in range(bc_len))   # base i at bits [2i, 2i+1]


@pytest.fixture(scope="module")
def counted(ia, ctx):
    """A few thousand seeded records, counted once: the {barcode, index, umi} records on the device, and count_np's COO."""
    n = 5000
    r = cnp.make_records(np.random.default_rng(0x3A7500), n, BC_LEN, 60, N_FEATURES, 12, high_bit=False)
    want, _ = cnp.count_matrix(r)
    assert int(want[1].max()) == N_FEATURES - 1 and (want[3] < want[2]).any()
    d, tmp = ctx.upload(r), ctx.alloc(24 * n)
    got = ctx.count_matrix(d, tmp, n, leave_swapped=True)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    tmp.free()
    yield d, n, want
    d.free()


def _want_coo(want, column, suffix=""):
    return [(_text(b) + suffix, int(i), int(v)) for b, i, v in zip(want[0], want[1], want[column])]


def test_write_matrix_market_reads_back_as_the_count_matrix(ctx, counted, tmp_path):
    d, n, want = counted
    out = tmp_path / "umis"
    rows = mtx_np.matrix_rows(want[0])[1]
    assert ctx.write_matrix_market(str(out), d, n, N_FEATURES, BC_LEN, piece_bytes=1000) == (len(rows), len(want[0]))
    nf, barcodes, features, coo = mtx_np.read_directory(str(out))
    assert nf == N_FEATURES and features == [str(j) for j in range(N_FEATURES)]
    assert barcodes == [_text(b) for b in rows] and coo == _want_coo(want, 3)
    assert sorted(os.listdir(out)) == ["barcodes.tsv", "features.tsv", "matrix.mtx"]


def test_write_matrix_market_reads_suffix_and_names(ctx, counted, tmp_path):
    d, n, want = counted
    names = [f"GENE{j}" for j in range(N_FEATURES)]
    ctx.write_matrix_market(str(tmp_path), d, n, N_FEATURES, BC_LEN, values="reads", barcode_suffix="-1", feature_names=names)
    nf, barcodes, features, coo = mtx_np.read_directory(str(tmp_path))
    assert features == names and all(b.endswith("-1") and len(b) == BC_LEN + 2 for b in barcodes)
    assert coo == _want_coo(want, 2, "-1")


def test_write_matrix_market_refuses_an_index_out_of_range_before_any_file(ctx, counted, tmp_path):
    d, n, want = counted
    with pytest.raises(ValueError):
        ctx.write_matrix_market(str(tmp_path), d, n, N_FEATURES - 1, BC_LEN)
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError):
        ctx.write_matrix_market(str(tmp_path / "never"), d, n, N_FEATURES - 1, BC_LEN)
    assert os.listdir(tmp_path) == []
    for kw in ({"values": "cells"}, {"feature_names": ["a"]}):
        with pytest.raises(ValueError):
            ctx.write_matrix_market(str(tmp_path), d, n, N_FEATURES, BC_LEN, **kw)
    assert os.listdir(tmp_path) == []


def test_matrix_csr_equals_the_csr_of_the_count_matrix(ctx, counted):
    d, n, want = counted
    _, keys, ptr = mtx_np.matrix_rows(want[0])
    for values, column in (("umis", 3), ("reads", 2)):
        m = ctx.matrix_csr(d, n, values=values)
        assert (m.n_rows, m.nnz) == (len(keys), len(want[0]))
        got = m.download()
        assert [g.tobytes() for g in got] == [keys.tobytes(), ptr.tobytes(), want[1].tobytes(), want[column].tobytes()]
        assert m.indptr.__cuda_array_interface__["data"][0] == m.indptr.ptr
        m.free()
    empty = ctx.matrix_csr(None, 0).download()
    assert [e.tolist() for e in empty] == [[], [0], [], []]


def test_count_file_example_writes_the_directory_it_prints(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    n = 20_000
    r = cnp.make_records(np.random.default_rng(0x3A7600), n, BC_LEN, 200, N_FEATURES, 12, high_bit=False)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(BC_LEN, 12))
    wr.write_batch(r)
    wr.finish()
    wr.close()
    for extra in ([], ["--cells=top:50"]):
        out = tmp_path / f"mtx{len(extra)}"
        out.mkdir()
        run = subprocess.run([str(exe), *extra, f"--mtx={out}", f"--n-features={N_FEATURES}", str(tmp_path / "in.ibu")], capture_output=True, text=True,
                             timeout=300)
        assert run.returncode == 0, run.stderr
        printed = [l.split("\t") for l in run.stdout.splitlines() if not l.startswith("#")]
        nf, barcodes, _, coo = mtx_np.read_directory(str(out))
        assert nf == N_FEATURES and len(printed) > 100 and coo == [(b, int(i), int(u)) for b, i, u, _ in printed]
        assert barcodes == [l.split("\t")[1] for l in run.stdout.splitlines() if l.startswith("#row\t")]
    out = tmp_path / "refused"
    out.mkdir()
    run = subprocess.run([str(exe), f"--mtx={out}", f"--n-features={N_FEATURES - 1}", str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and "not below" in run.stderr and os.listdir(out) == []
