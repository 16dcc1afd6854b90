"""The per-row top-2 and the row class on the device (ibu_matrix_row_top, ibu_assign_rows): every comparison is byte for byte against
the numpy / Python statement of the semantics in tests/rowtop_np.py; every call goes through the C ABI, and every buffer — the
columns at exactly 8 B per entry, the bitmap at exactly its words, each output at exactly 8 B per row, the class bytes at 1 B per row —
is carved at its contract size out of the guard-zone arena of tests/test_gpu_count.py.  The input columns are compared after every
case: they are never written.  One test per size, its shapes inside it: a case is milliseconds."""
import ctypes as C

import numpy as np
import pytest

from tests import count_np as cnp
from tests import rowtop_np as rt
from tests.test_gpu_count import PATTERN, _arena, _p
from tests.test_gpu_mtx import ROW_SHAPES, SIZES, UNIT, _row_shape
from tests.test_gpu_sweeps import _context, _units, cus  # noqa: F401  (cus: a fixture, on this module's ia and ctx)

pytestmark = pytest.mark.gpu

FINISH_LANES = 64                                                # k_matrix.hip kTopFinishLanes: following units one step of the finishing wave takes
GARBAGE = 0x5A5A5A5A5A5A5A5A
TOP = (1 << 64) - 1
U = np.uint64
LONG = (UNIT - 700, 2 * UNIT + 500)                              # the row that spans exactly three units: 700 entries, a whole unit, 500
SHAPES = ROW_SHAPES + ["three_units"]
VALUES = ["equal", "ascending", "descending", "random8", "wrap", "zeros"]
SETS = ["none", "all", "every_other", "without_max", "empty_rows", "bits_below_keys", "alias"]
NAMES = ("top_key", "top_value", "next_value", "row_sum", "row_entries")


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _top(ia, ctx, cols, n, d_set, bits, outs, cap, stream=None):
    """One ibu_matrix_row_top call through the C ABI -> *n_rows; outs = the five outputs, DeviceBuffers or None."""
    nr = C.c_size_t(12345)
    ia._check(ia.lib.ibu_matrix_row_top(ctx._c, *[_p(c) for c in cols], n, _p(d_set), bits, *[_p(o) for o in outs], cap, C.byref(nr), stream))
    return nr.value


def _dl(buf, words):
    return buf.download(np.uint64, words) if words else np.empty(0, np.uint64)


def _first(shape, n, seed=0):
    if shape != "three_units":
        return _row_shape(shape, n, seed)
    rng = np.random.default_rng(0x70B300 + n)                    # rows of 1 .. 8 entries on either side of the long row
    row = np.repeat(np.arange(n + 1, dtype=np.uint64), rng.integers(1, 9, n + 1))[:n]
    a, b = LONG
    if n > a:
        row[a:min(b, n)] = row[a] + U(1 << 40)                    # one value over [a, b): its neighbours differ from it
    return row[:n]


def _values(pattern, n):
    i = np.arange(n, dtype=np.uint64)
    if pattern == "equal":
        return np.full(n, 5, np.uint64)
    if pattern == "ascending":
        return i + U(1)
    if pattern == "descending":
        return U(n) - i
    if pattern == "random8":                                     # many ties and zeros
        return np.random.default_rng(0x70B400 + n).integers(0, 8, n).astype(np.uint64)
    if pattern == "wrap":                                        # 2^64 - 1 and 2^63: the sums wrap
        return np.where(i % U(3) == 0, U(TOP), U(1 << 63))
    return np.zeros(n, np.uint64)


def _keys_and_set(kind, first, values):
    """-> (second, None | (bitmap words, set_bits))."""
    n = len(first)
    i = np.arange(n, dtype=np.uint64)
    second = i % U(60)
    if kind == "none":
        return second, None
    if kind == "all":
        return second, (rt.bitmap(range(60), 60), 60)
    if kind == "every_other":
        return second, (rt.bitmap(range(0, 60, 2), 60), 60)
    if kind == "without_max":                                    # the first largest entry of every row gets the one key outside the set
        at = rt.row_top(first, i, values)[0].astype(np.int64)
        second[at] = 60
        return second, (rt.bitmap(range(60), 60), 60)
    if kind == "empty_rows":                                     # whole rows outside the set: the first, the last, the one at a unit seam, every fifth
        starts = rt.row_starts(first)
        row = np.repeat(np.arange(len(starts)), np.diff(np.concatenate([starts, [n]])))
        gone = row % 5 == 3
        for k in (0, n - 1, min(UNIT, n - 1), min(UNIT - 1, n - 1)):
            if n:
                gone |= row == row[k]
        second[gone] = 63
        return second, (rt.bitmap(range(60), 64), 64)
    if kind == "bits_below_keys":                                # keys 37 .. 59 are not below set_bits
        return second, (rt.bitmap([v for v in range(37) if v % 3], 37), 37)
    second = np.where(i % U(3) == 0, second + U(1 << 32), second)   # 2^32 + j with bit j set: never bit j
    return second, (rt.bitmap(range(60), 60), 60)


def _check_case(ia, ctx, first, second, values, fset, label, stream=None):
    n = len(first)
    words, bits = fset if fset is not None else (None, 0)
    want = rt.row_top(first, second, values, words, bits)
    r = len(want[0])
    ar = _arena(ia, ctx, 8 * n, 8 * n, 8 * n, 8 * (len(words) if words is not None else 0), *[8 * r] * 5)
    try:
        d_cols = [ar.carve(8 * n, 8 * (k & 1)) for k in range(3)]
        for d, c in zip(d_cols, (first, second, values)):
            if n:
                d.upload(c)
        d_set = None
        if words is not None:
            d_set = ar.carve(8 * len(words), 8)
            d_set.upload(words)
        outs = [ar.carve(8 * r, 8 * (k & 1)) for k in range(5)]
        given = [None] * 3 if n == 0 else d_cols
        assert _top(ia, ctx, given, n, d_set, bits, [None] * 5, 0, stream) == r, label          # the size query
        assert _top(ia, ctx, given, n, d_set, bits, outs, r, stream) == r, label                # cap == n_rows exactly
        if stream is not None:
            ctx.synchronize(stream)
        ar.check(label)
        for name, o, w in zip(NAMES, outs, want):
            g = _dl(o, r)
            assert g.tobytes() == w.tobytes(), (label, name, np.flatnonzero(g != w)[:5], g[g != w][:5], w[g != w][:5])
        for d, c in zip(d_cols, (first, second, values)):
            assert _dl(d, n).tobytes() == c.tobytes(), label
        if words is not None:
            assert _dl(d_set, len(words)).tobytes() == words.tobytes(), label
    finally:
        ar.free()
    return want


@pytest.mark.parametrize("n", SIZES)
def test_row_top_matches_numpy(ia, ctx, n):
    k = 0
    for shape in SHAPES:
        first = _first(shape, n)
        for pattern in VALUES:
            values = _values(pattern, n)
            kind = SETS[k % len(SETS)]                           # 6 patterns, 7 sets: every pair of them meets over the shapes
            k += 1
            second, fset = _keys_and_set(kind, first, values)
            want = _check_case(ia, ctx, first, second, values, fset, f"n={n} {shape} {pattern} set={kind}")
            if n and kind == "none" and pattern == "equal":      # the row's first entry, and next == top where the row has two
                starts = rt.row_starts(first)
                assert (want[0] == second[starts]).all() and (want[2][want[4] > 1] == 5).all() and (want[2][want[4] == 1] == 0).all()
            if n and kind == "none" and pattern == "zeros":
                assert (want[0] == second[rt.row_starts(first)]).all() and not want[1].any()
                assert (rt.assign(want[1], want[2], want[3], 0, 0, 1)[0] == rt.ROW_NONE).all()


def test_three_units_shape_has_the_row_it_names():
    first = _first("three_units", 3 * UNIT + 1)
    starts = rt.row_starts(first).tolist()
    assert LONG[0] in starts and LONG[1] in starts and not any(LONG[0] < s < LONG[1] for s in starts)
    assert LONG[0] // UNIT == 0 and (LONG[1] - 1) // UNIT == 2 and max(np.diff(starts[:starts.index(LONG[0]) + 1])) <= 8


@pytest.mark.parametrize("kind", SETS)
def test_row_top_every_set_on_every_shape(ia, ctx, kind):
    for n in (3 * UNIT + 1, 16 * UNIT + 1):
        for shape in SHAPES:
            first = _first(shape, n)
            values = _values("random8", n)
            second, fset = _keys_and_set(kind, first, values)
            want = _check_case(ia, ctx, first, second, values, fset, f"n={n} {shape} set={kind}")
            if kind == "empty_rows":
                assert want[4][0] == 0 and want[4][-1] == 0 and (want[0][want[4] == 0] == rt.NO_KEY).all()


def test_row_top_a_row_longer_than_one_step_of_the_finishing_wave(ia, ctx):
    """FINISH_LANES + 2 units in one row, between short rows: the finishing wave of the row's first unit takes a second step, and
    every lane but two has folded one partial in before the reduction over the lanes."""
    n = (FINISH_LANES + 3) * UNIT + 1
    first = _first("random", n).copy()
    first[UNIT - 5:(FINISH_LANES + 2) * UNIT + 9] = 3
    for pattern in ("equal", "ascending", "descending", "random8"):
        values = _values(pattern, n)
        for kind in ("none", "every_other"):
            second, fset = _keys_and_set(kind, first, values)
            _check_case(ia, ctx, first, second, values, fset, f"long row {pattern} {kind}")


PARTS = {"head": LONG[0] + 50, "middle": UNIT + 1000, "tail": 2 * UNIT + 400}


@pytest.mark.parametrize("top_in", sorted(PARTS))
def test_row_top_single_maximum_in_every_part_of_a_three_unit_row(ia, ctx, top_in):
    n = 3 * UNIT + 77
    first = _first("three_units", n)
    second = np.arange(n, dtype=np.uint64) % U(60)
    row = int(np.searchsorted(rt.row_starts(first), LONG[0]))
    for next_in in [None] + [p for p in sorted(PARTS) if p != top_in]:
        values = np.ones(n, np.uint64)
        values[PARTS[top_in]] = 9
        if next_in:
            values[PARTS[next_in]] = 5
        want = _check_case(ia, ctx, first, second, values, None, f"maximum in the {top_in}, runner-up in the {next_in}")
        assert [int(w[row]) for w in want] == [PARTS[top_in] % 60, 9, 5 if next_in else 1, LONG[1] - LONG[0] + 8 + (4 if next_in else 0), LONG[1] - LONG[0]]


def test_row_top_forms_of_the_call(ia, ctx):
    n = 3 * UNIT + 77
    first = _first("random", n)
    values = _values("random8", n)
    second, (words, bits) = _keys_and_set("every_other", first, values)
    want = rt.row_top(first, second, values, words, bits)
    r = len(want[0])
    ar = _arena(ia, ctx, 8 * n, 8 * n, 8 * n, 8 * len(words), *[8 * r] * 10)
    try:
        d_cols = [ar.carve(8 * n, 0) for _ in range(3)]
        for d, c in zip(d_cols, (first, second, values)):
            d.upload(c)
        d_set = ar.carve(8 * len(words), 0)
        d_set.upload(words)
        for k in range(5):                                       # each output alone
            out = ar.carve(8 * r, 0)
            assert _top(ia, ctx, d_cols, n, d_set, bits, [out if j == k else None for j in range(5)], r) == r
            ar.check(f"output {k} alone")
            assert _dl(out, r).tobytes() == want[k].tobytes(), NAMES[k]
        outs = [ar.carve(8 * r, 0) for _ in range(5)]
        untouched = lambda: all((o.download(np.uint8, 8 * r) == PATTERN).all() for o in outs)
        assert _top(ia, ctx, d_cols, n, d_set, bits, [None] * 5, 5) == r          # the size query, whatever cap says
        nr = C.c_size_t(12345)                                   # cap one too small: refused, *n_rows set, nothing written
        rc = ia.lib.ibu_matrix_row_top(ctx._c, *[_p(c) for c in d_cols], n, _p(d_set), bits, *[_p(o) for o in outs], r - 1, C.byref(nr), None)
        with pytest.raises(ia.IbuError) as ei:
            ia._check(rc)
        assert ei.value.kind == "InvalidArg" and (ei.value.a, ei.value.b) == (r, r - 1) and nr.value == r
        ar.check("cap one too small")
        assert untouched()
        refused = [(d_cols, n, None, 60, outs, r),                                                  # no set, and set_bits not 0
                   (d_cols, n, d_set, (1 << 32) + 1, outs, r),                                      # more bits than a bitmap may have
                   ([None, d_cols[1], d_cols[2]], n, d_set, bits, outs, r),                         # a NULL column
                   ([d_cols[0], C.c_void_p(d_cols[1].ptr + 4), d_cols[2]], n, d_set, bits, outs, r),  # a misaligned column
                   (d_cols, 1 << 40, d_set, bits, outs, r),                                         # too many entries
                   (d_cols, n, d_set, bits, [outs[0], C.c_void_p(outs[1].ptr + 4)] + outs[2:], r),  # a misaligned output
                   (d_cols, n, d_set, bits, [outs[0], outs[0]] + outs[2:], r),                      # two outputs are one array
                   (d_cols, n, d_set, bits, [d_cols[2]] + outs[1:], r)]                             # an output is an input column
        for cols, count, s, b, o, cap in refused:
            raw = lambda x: x if isinstance(x, C.c_void_p) or x is None else _p(x)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_matrix_row_top(ctx._c, *[raw(c) for c in cols], count, raw(s), b, *[raw(x) for x in o], cap, C.byref(nr), None))
            assert ei.value.kind == "InvalidArg"
        with pytest.raises(ia.IbuError):
            ia._check(ia.lib.ibu_matrix_row_top(ctx._c, *[_p(c) for c in d_cols], n, _p(d_set), bits, *[None] * 5, 0, None, None))   # n_rows is NULL
        ar.check("refused calls")
        assert untouched()
        for d, c in zip(d_cols, (first, second, values)):
            assert _dl(d, n).tobytes() == c.tobytes()
        assert _top(ia, ctx, [None] * 3, 0, None, 0, outs, r) == 0               # no entries: nothing touched
        assert untouched()
        other = ia.Context(0)                                    # a stream of the caller's: another context's
        try:
            assert _top(ia, ctx, d_cols, n, d_set, bits, outs, r, other.stream) == r
            other.synchronize()
        finally:
            other.close()
        ar.check("on a side stream")
        assert [_dl(o, r).tobytes() for o in outs] == [w.tobytes() for w in want]
        same = rt.row_top(first, first, first)                   # the three input columns may be one array
        assert _top(ia, ctx, [d_cols[0]] * 3, n, None, 0, outs, r) == r
        ar.check("one column three times")
        assert [_dl(o, r).tobytes() for o in outs] == [w.tobytes() for w in same]
        # the Python wrapper
        top = ctx.matrix_row_top(*d_cols, n, feature_set=(d_set, bits))
        assert top.n_rows == r and [g.tobytes() for g in top.download()] == [w.tobytes() for w in want]
        top.free()
        empty = ctx.matrix_row_top(None, None, None, 0)
        assert empty.n_rows == 0 and [len(g) for g in empty.download()] == [0] * 5
    finally:
        ar.free()


# ---- the class of a row ------------------------------------------------------------------------------------------------
B63 = 1 << 63
# (top, next, sum) by hand.  Under (min 1, share 2/3): equality, one below equality, the same two where the products pass 2^64,
# a tied top whose share would pass, no entry at all, a top of 1, a sum that wrapped to less than the top.
HAND = [(6, 3, 9), (5, 3, 8), (B63, 1, 3 << 62), (B63, 1, (3 << 62) + 1), (5, 5, 7), (0, 0, 0), (1, 0, 1), (TOP, B63, B63 - 1), (B63, 0, B63),
        (B63, 1, B63 + 1), (7, 2, 30), (2, 1, 3), (TOP, TOP, 5), (TOP, 0, TOP)]   # the last two: mixed and assigned under every rule
RULES = [(1, 2, 3), (1, 0, 1), (0, 0, 1), (0, 3, 3), (6, 1, 1), (TOP, 1, 2), (2, 1, 3)]
ASSIGN_SIZES = [0, 1, 63, 64, 65, 100_003]


def _assign(ia, ctx, cols, rows, rule, d_class, want_counts, stream=None):
    """One ibu_assign_rows call through the C ABI -> the counts as a dict, or None."""
    from ibu_amd import _lib
    c = _lib.CAssignCounts(GARBAGE, GARBAGE, GARBAGE, GARBAGE) if want_counts else None
    r = _lib.CAssignRule(*rule)
    ia._check(ia.lib.ibu_assign_rows(ctx._c, *[_p(x) for x in cols], rows, C.byref(r), _p(d_class), C.byref(c) if want_counts else None, stream))
    return {f: int(getattr(c, f)) for f in ("rows", "assigned", "none", "mixed")} if want_counts else None


@pytest.mark.parametrize("rows", ASSIGN_SIZES)
def test_assign_rows_matches_python(ia, ctx, rows):
    hand = np.array([HAND[k % len(HAND)] for k in range(rows)], dtype=np.uint64).reshape(rows, 3)
    host = [np.ascontiguousarray(hand[:, k]) for k in range(3)]
    ar = _arena(ia, ctx, 8 * rows, 8 * rows, 8 * rows, rows)
    try:
        cols = [ar.carve(8 * rows, 8 * (k & 1)) for k in range(3)]
        for d, h in zip(cols, host):
            if rows:
                d.upload(h)
        d_class = ar.carve(rows, 3)
        given = cols if rows else [None] * 3
        for rule in RULES:
            cls, counts = rt.assign(*host, *rule)
            if rows >= 64:
                assert counts["assigned"] and counts["none"] and counts["mixed"], counts   # a kernel that writes one class everywhere fails
            assert _assign(ia, ctx, given, rows, rule, d_class, True) == counts, rule     # both
            ar.check(f"rule {rule}")
            if rows:
                assert d_class.download(np.uint8, rows).tobytes() == cls.tobytes(), rule
                d_class.upload(np.full(rows, PATTERN, np.uint8))
            assert _assign(ia, ctx, given, rows, rule, None, True) == counts, rule        # the counts only
            if rows:
                assert (d_class.download(np.uint8, rows) == PATTERN).all()
            assert _assign(ia, ctx, given, rows, rule, d_class, False) is None            # the classes only
            ar.check(f"rule {rule}, classes only")
            if rows:
                assert d_class.download(np.uint8, rows).tobytes() == cls.tobytes(), rule
        for d, h in zip(cols, host):
            assert _dl(d, rows).tobytes() == h.tobytes()
    finally:
        ar.free()


def test_assign_rows_by_hand_and_refused_calls(ia, ctx):
    from ibu_amd import _lib
    rows = len(HAND)
    host = [np.array([h[k] for h in HAND], np.uint64) for k in range(3)]
    A, N, M = rt.ROW_ASSIGNED, rt.ROW_NONE, rt.ROW_MIXED
    by_hand = {(1, 2, 3): [A, M, A, M, M, N, A, A, A, A, M, A, M, A],   # equality passes, one below does not, in 64 bits and beyond
               (1, 0, 1): [A, A, A, A, M, N, A, A, A, A, A, A, M, A],   # no share test: top > next decides
               (0, 0, 1): [A, A, A, A, M, N, A, A, A, A, A, A, M, A],   # min_value 0 still wants a top of 1
               (0, 3, 3): [M, M, M, M, M, N, A, A, A, M, M, M, M, A]}   # the whole sum: 3 * 2^63 against 3 * (2^63 + 1)
    ar = _arena(ia, ctx, 8 * rows, 8 * rows, 8 * rows, rows)
    try:
        cols = [ar.carve(8 * rows, 0) for _ in range(3)]
        for d, h in zip(cols, host):
            d.upload(h)
        d_class = ar.carve(rows, 1)
        for rule, want in by_hand.items():
            assert rt.assign(*host, *rule)[0].tolist() == want, rule
            counts = _assign(ia, ctx, cols, rows, rule, d_class, True)
            assert d_class.download(np.uint8, rows).tolist() == want, rule
            assert counts == {"rows": rows, "assigned": want.count(A), "none": want.count(N), "mixed": want.count(M)}
        d_class.upload(np.full(rows, PATTERN, np.uint8))
        c = _lib.CAssignCounts(GARBAGE, GARBAGE, GARBAGE, GARBAGE)
        ok = _lib.CAssignRule(1, 2, 3)
        calls = [(cols, C.byref(_lib.CAssignRule(1, 4, 3)), d_class, C.byref(c)),      # num > den
                 (cols, C.byref(_lib.CAssignRule(1, 0, 0)), d_class, C.byref(c)),      # den == 0
                 (cols, None, d_class, C.byref(c)),                                    # no rule
                 (cols, C.byref(ok), None, None),                                      # nothing to do
                 ([None, cols[1], cols[2]], C.byref(ok), d_class, C.byref(c)),         # a NULL column
                 ([cols[0], C.c_void_p(cols[1].ptr + 4), cols[2]], C.byref(ok), d_class, C.byref(c))]   # a misaligned column
        for given, rule, cls, counts in calls:
            raw = lambda x: x if isinstance(x, C.c_void_p) or x is None else _p(x)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_assign_rows(ctx._c, *[raw(x) for x in given], rows, rule, raw(cls), counts, None))
            assert ei.value.kind == "InvalidArg"
        ar.check("refused calls")
        assert (d_class.download(np.uint8, rows) == PATTERN).all() and [c.rows, c.assigned, c.none, c.mixed] == [GARBAGE] * 4
    finally:
        ar.free()


# ---- end to end, and the sweep -----------------------------------------------------------------------------------------
def test_assign_features_equals_numpy_on_the_count_matrix(ia, ctx):
    n, n_features = 5000, 40
    hashtags = [3, 7, 8, 15, 22, 23, 31, 39]
    r = cnp.make_records(np.random.default_rng(0x70B500), n, 16, 36, n_features, 12, high_bit=False)
    (barcodes, indices, reads, umis), _ = cnp.count_matrix(r)
    d, tmp = ctx.upload(r), ctx.alloc(24 * n)
    ctx.count_matrix(d, tmp, n, leave_swapped=True)
    fset = ctx.feature_bitmap(hashtags, n_features)
    for values, column, rule in (("umis", umis, dict(min_value=3, min_share=(1, 2))), ("reads", reads, dict(min_value=1))):
        want = rt.row_top(barcodes, indices, column, rt.bitmap(hashtags, n_features), n_features)
        cls, counts = rt.assign(want[1], want[2], want[3], rule["min_value"], *rule.get("min_share", (0, 1)))
        d_keys, top, d_class, got_counts = ctx.assign_features(d, n, feature_set=fset, values=values, **rule)
        rows = top.n_rows
        assert rows == len(want[0]) and got_counts == ia.AssignCounts(**counts)
        assert d_keys.download(np.uint64, rows).tobytes() == barcodes[rt.row_starts(barcodes)].tobytes()
        assert [g.tobytes() for g in top.download()] == [w.tobytes() for w in want]
        assert d_class.download(np.uint8, rows).tobytes() == cls.tobytes()
        assert set(want[0].tolist()) <= set(hashtags) | {rt.NO_KEY}
        top.free()
    assert len(set(cls.tolist())) >= 2
    for b in (d, tmp, fset[0]):
        b.free()


def test_row_top_over_two_units_per_wave(ia, cus):  # noqa: F811
    """blocks_per_cu = 1 and the unit count of tests/test_gpu_sweeps.py: every wave of the reduce pass handles at least one unit and
    many two, and with one row over the whole table the finishing pass meets a row that is open across every unit."""
    c = _context(ia)
    try:
        n, plan = _units(cus)
        values = _values("random8", n)
        for shape in ("random", "rows_2049", "one_row"):
            first = _first(shape, n)
            for kind in ("none", "every_other"):
                second, fset = _keys_and_set(kind, first, values)
                _check_case(ia, c, first, second, values, fset, f"n={n} {shape} set={kind}")
    finally:
        c.close()
