"""Per-barcode labels onto records on the device (ibu_labels_create / _set / _get, ibu_label_records): every comparison is byte for
byte against the numpy statement of the semantics in tests/label_np.py — class bytes, the 257-bin histogram, the labels read back
and the number of codes skipped.  The buffers are carved at contract size from the guard arena of tests/test_gpu_resolve.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import count_np as cnp
from tests import label_np as lnp
from tests import rowtop_np as rt
from tests import sweep_np as sw
from tests import whitelist_np as wnp
from tests.test_gpu_resolve import PATTERN, Arena, _arena, _whitelist
from tests.test_gpu_sweeps import REST, _context, _shape, _traced, cus  # noqa: F401  (cus: a fixture, on this module's ia and ctx)

pytestmark = pytest.mark.gpu

NS = [0, 1, 127, 128, 129, 5121, 100_003]
BC_LENS = [5, 16, 32]
WS = [2, 1000, 100_000]
CASES = [(b, w, n) for b, w, n in itertools.product(BC_LENS, WS, NS) if 4 ** b >= w]   # the only pruning: a whitelist larger than the code space
CLASS_SKEWS = [0, 1, 2, 15]
MODES = [(None, 255), (None, 3), (0, 255), (7, 255), (200, 255)]                       # (match, missing_class)
OUTPUTS = ["both", "class", "hist"]
FILL = 201
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


def _p(buf):
    return C.c_void_p(buf.ptr) if buf is not None else None


def _label(ia, ctx, lb, d, n, match, missing_class, d_cls, want_hist):
    """ibu_label_records through the C ABI -> the histogram as numpy u64[257] (None when not asked for)."""
    h = (C.c_uint64 * 257)(*([GARBAGE] * 257)) if want_hist else None
    ia._check(ia.lib.ibu_label_records(ctx._c, lb._c, _p(d), n, 0 if match is None else ia.LABEL_MATCH, 0 if match is None else match,
                                       missing_class, _p(d_cls), h, None))
    return np.array(h, dtype=np.uint64) if want_hist else None


@functools.lru_cache(maxsize=4)
def _case(bc_len, w):
    """The whitelist of a (bc_len, w) cell and the largest input in either order; the smaller sizes are prefixes."""
    rng = np.random.default_rng(0x1AB0200 + 1000 * bc_len + w % 997)
    wl = lnp.whitelist(rng, bc_len, w, ones=bc_len == 32 and w == 1000)      # one cell has the all-ones key as an entry
    recs = {order: lnp.records(rng, lnp.barcodes(rng, wl, bc_len, max(NS), order)) for order in ("shuffled", "sorted")}
    if bc_len == 32:
        for r in recs.values():
            at = np.concatenate([[50], rng.integers(500, len(r), 200)])          # behind the planted runs, and one in the small prefixes
            r["barcode"][at] = np.uint64(wnp.FREE)                               # read in every 32-base cell, an entry in one
    return wl, recs


def _check_all(ia, ctx, ar, lb, lb_np, d, recs, n, d_classes, what):
    """Every mode and every choice of outputs on one array of records, the class skew rotating; `ar` checked after every call."""
    fill = np.full(max(n, 1), PATTERN, np.uint8)
    k = 0
    for match, missing_class in MODES:
        cls_np, hist_np = lnp.label_records(lb_np, recs, match, missing_class)
        assert int(hist_np.sum()) == n
        for out in OUTPUTS:
            skew = CLASS_SKEWS[k % len(CLASS_SKEWS)]
            k += 1
            d_cls = d_classes[skew]
            if n:
                d_cls.upload(fill)
            hist = _label(ia, ctx, lb, d, n, match, missing_class, d_cls if out != "hist" else None, out != "class")
            where = (what, match, missing_class, out, skew)
            ar.check(str(where))
            got = d_cls.download(np.uint8, max(n, 1))[:n]
            if out == "hist":
                assert (got == PATTERN).all(), where
            else:
                assert got.tobytes() == cls_np.tobytes(), where
            if out != "class":
                assert hist.tobytes() == hist_np.tobytes(), where


@pytest.mark.parametrize("bc_len,w,n", CASES)
def test_label_records_matches_numpy(ia, ctx, bc_len, w, n):
    """Records whose base is 8 but not 16 bytes aligned (one record is peeled), the class bytes 0, 1, 2 and 15 bytes behind a
    16-byte boundary; shuffled and sorted with long runs, about a tenth of the records not in the whitelist, upper barcode bits set;
    three label patterns."""
    wl, by_order = _case(bc_len, w)
    ar = _arena(ia, ctx, 24 * n, 24 * n, *([n] * len(CLASS_SKEWS)))
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h:
            d_classes = {s: ar.carve(n, s) for s in CLASS_SKEWS}
            for order, full in by_order.items():
                recs = full[:n]
                d = ar.carve(24 * n, 8)
                if n:
                    d.upload(recs)
                for pattern in lnp.PATTERNS:
                    codes, labs = lnp.label_pattern(wl, pattern)
                    lb_np = lnp.Labels(wl, bc_len, FILL)
                    assert lnp.set_labels(lb_np, codes, labs) == 0
                    with h.labels(fill=FILL) as lb:
                        assert lb.device_bytes >= h.n_distinct + 1
                        assert lb.set(codes, labs) == 0
                        _check_all(ia, ctx, ar, lb, lb_np, d, recs, n, d_classes, (order, pattern))
                if n:
                    assert d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are never written"
    finally:
        ar.free()


def test_the_patterns_reach_what_they_are_for():
    """rank256 reaches all 256 labels and leaves entries at fill; the sorted order holds a run of 300 and one that ends at record 128."""
    wl, by_order = _case(16, 1000)
    codes, labs = lnp.label_pattern(wl, "rank256")
    lb = lnp.Labels(wl, 16, FILL)
    lnp.set_labels(lb, codes, labs)
    assert set(lb.lab.tolist()) == set(range(256)) and len(codes) < len(lb.wl)
    cls, hist = lnp.label_records(lb, by_order["shuffled"])
    assert (hist[:256] > 0).all() and 0.05 < hist[256] / hist.sum() < 0.15
    low = by_order["sorted"]["barcode"] & wnp.mask(16)
    assert (low != by_order["sorted"]["barcode"]).any(), "upper barcode bits are set on some records"
    assert (low[128:428] == low[128]).all() and low[127] != low[128] and (low[100:128] == low[100]).all() and np.isin(low[128], wl)
    assert set(lnp.label_pattern(wl, "low8")[1].tolist()) == set(range(8))


# ---- several tiles per wave ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx(ia):
    c = _context(ia)                                             # blocks_per_cu = 1: the grid of a tiled kernel is min(ceil(ntiles / 4), cus)
    yield c
    c.close()


def _sweep_case(ia, ctx, capfd, n, ntiles, head, skew, what):
    bc_len = 16
    rng = np.random.default_rng([0x1AB0300, n])
    wl = lnp.whitelist(rng, bc_len, 1000)
    codes, labs = lnp.label_pattern(wl, "rank256")
    lb_np = lnp.Labels(wl, bc_len, FILL)
    lnp.set_labels(lb_np, codes, labs)
    ar = _arena(ia, ctx, 24 * n, n)
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, h.labels(fill=FILL) as lb:
            lb.set(codes, labs)
            d, d_cls = ar.carve(24 * n, skew), ar.carve(n, 1 if skew else 0)
            for order in ("shuffled", "sorted"):
                recs = lnp.records(rng, lnp.barcodes(rng, wl, bc_len, n, order))
                d.upload(recs)
                for match, want_cls in ((None, True), (7, True), (None, False)):
                    cls_np, hist_np = lnp.label_records(lb_np, recs, match, 255)
                    d_cls.upload(np.full(n, PATTERN, np.uint8))
                    hist, rows = _traced(ctx, capfd, lambda: _label(ia, ctx, lb, d, n, match, 255, d_cls if want_cls else None, True))
                    ar.check(f"{what} {order} match={match}")
                    assert len(rows) == 1 and rows[0]["tiled"] == ntiles * 128 and rows[0]["head"] == head and rows[0]["tile"] == 128, rows
                    assert hist.tobytes() == hist_np.tobytes(), (what, order, match)
                    got = d_cls.download(np.uint8, n)
                    assert got.tobytes() == cls_np.tobytes() if want_cls else (got == PATTERN).all()
                assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        ar.free()


@pytest.mark.parametrize("skew", [0, 8])
def test_histogram_over_three_and_four_tiles_per_wave(ia, small_ctx, capfd, cus, skew):
    """The shrunken grid of tests/test_gpu_sweeps.py: every wave sweeps three or four tiles, so a workgroup's LDS histogram collects
    twelve to sixteen tiles before its one flush.  Sized by that file's `_shape` — the 3/4 shape of the kernels with 128-row tiles,
    as for correct and abundance add — not by `_units`, which sizes the 2048-row unit loops at one and two units per wave."""
    head = 1 if skew else 0
    n, ntiles, plan = _shape("label records", cus, 128, head)
    _sweep_case(ia, small_ctx, capfd, n, ntiles, head, skew, "3/4 tiles")


def _empty_workgroups(plan):
    return [b for b in range(len(plan) // 4) if not any(plan[4 * b + k] for k in range(4))]


@pytest.mark.parametrize("skew", [0, 8])
def test_histogram_with_waves_that_get_no_tile(ia, small_ctx, capfd, cus, skew):
    """61 tiles: a grid of 16 workgroups, every XCD's part has 8 tiles but the last, which has 5 — three waves of its second
    workgroup get no tile and must still take part in the workgroup's clear, barrier and flush."""
    ntiles = 61
    plan = sw.sweep_plan(cus, 1, ntiles)
    empty = [k for k, w in enumerate(plan) if not w]
    assert len(plan) == 64 and empty == [61, 62, 63] and not _empty_workgroups(plan), empty
    head = 1 if skew else 0
    _sweep_case(ia, small_ctx, capfd, head + ntiles * 128 + REST, ntiles, head, skew, "waves without a tile")


@pytest.mark.parametrize("skew", [0, 8])
def test_histogram_with_workgroups_that_get_no_tile(ia, small_ctx, capfd, cus, skew):
    """One tile past the cap of the grid, 4 cus + 1 tiles on cus workgroups: the static XCD split gives every part ceil(ntiles / 8)
    tiles, the last part is what is left, seven tiles short, and the last workgroup of the last XCD starts behind its end — on 256
    CUs tile_range(256, 255, 0, 1025) begins at tile 1027.  That workgroup's four waves have no tile; they clear the LDS histogram,
    reach the barrier and flush nothing, while the other workgroups of the part sweep one or two tiles.  The mirror of the launch
    plan (tests/sweep_np.py) names the empty workgroups; a device whose CU count is no multiple of 8 takes the stride form, which
    has none, and the case then runs as one more size."""
    ntiles = 4 * cus + 1
    plan = sw.sweep_plan(cus, 1, ntiles)
    empty = _empty_workgroups(plan)
    assert len(plan) == 4 * cus and sorted(t for w in plan for t in w) == list(range(ntiles))
    assert bool(empty) == (cus % 8 == 0), (cus, empty)
    if cus == 256:
        assert empty == [255] and sw.tile_range(256, 255, 0, 1025)[0] == 1027
    head = 1 if skew else 0
    _sweep_case(ia, small_ctx, capfd, head + ntiles * 128 + REST, ntiles, head, skew, "workgroups without a tile")


# ---- set and get -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc_len", BC_LENS)
def test_set_and_get(ia, ctx, bc_len):
    """Two set calls, the second overriding half of the first; get over all entries, their one-base neighbours and, below 32 bases,
    codes with a bit above 2*bc_len; the label bytes at odd addresses."""
    rng = np.random.default_rng([0x1AB0400, bc_len])
    wl = lnp.whitelist(rng, bc_len, 1000 if bc_len > 5 else 600, ones=bc_len == 32)
    u = np.unique(wl)
    out = lnp.outsiders(rng, wl, bc_len, 50)
    first_codes = rng.permutation(np.concatenate([u[: len(u) * 3 // 4], out]))
    if bc_len < 32:
        first_codes = np.concatenate([first_codes, u[:5] | np.uint64(1 << (2 * bc_len))])
    if bc_len == 32:
        first_codes = np.concatenate([first_codes, [np.uint64(wnp.FREE)]])    # the entry whose label lives outside the table
    first_labs = rng.integers(0, 256, len(first_codes)).astype(np.uint8)
    second_codes = rng.permutation(u[len(u) * 3 // 8: len(u) * 7 // 8])       # half of the first call's entries, and an eighth never set
    second_labs = rng.integers(0, 256, len(second_codes)).astype(np.uint8)
    probe = np.concatenate([u, u ^ np.uint64(1), u ^ np.uint64(2 << (2 * (bc_len - 1)))] + ([u[:64] | np.uint64(1 << (2 * bc_len))] if bc_len < 32 else []))
    lb_np = lnp.Labels(wl, bc_len, FILL)
    skipped_np = [lnp.set_labels(lb_np, first_codes, first_labs), lnp.set_labels(lb_np, second_codes, second_labs)]
    assert skipped_np[0] >= 50 and skipped_np[1] == 0 and (lb_np.lab == FILL).sum() >= len(u) // 8
    k1, k2, kp = len(first_codes), len(second_codes), len(probe)
    ar = _arena(ia, ctx, 8 * k1, k1, 8 * k2, k2, 8 * kp, kp)
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, h.labels(fill=FILL) as lb:
            d_c1, d_l1, d_c2, d_l2 = ar.carve(8 * k1), ar.carve(k1, 3), ar.carve(8 * k2), ar.carve(k2, 1)
            d_probe, d_out = ar.carve(8 * kp), ar.carve(kp, 5)
            d_c1.upload(first_codes); d_l1.upload(first_labs); d_c2.upload(second_codes); d_l2.upload(second_labs); d_probe.upload(probe)
            skipped = C.c_size_t(77)
            ia._check(ia.lib.ibu_labels_set(ctx._c, lb._c, _p(d_c1), _p(d_l1), k1, C.byref(skipped), None))
            assert skipped.value == skipped_np[0]
            ia._check(ia.lib.ibu_labels_set(ctx._c, lb._c, _p(d_c2), _p(d_l2), k2, None, None))          # asynchronous, in stream order
            ia._check(ia.lib.ibu_labels_get(ctx._c, lb._c, _p(d_probe), kp, 9, _p(d_out), None))
            ar.check("set, set, get")
            assert d_out.download(np.uint8, kp).tobytes() == lnp.get_labels(lb_np, probe, 9).tobytes()
            assert (lb.get(probe, missing=255) == lnp.get_labels(lb_np, probe, 255)).all()
            # k == 0 is OK and touches nothing
            skipped = C.c_size_t(77)
            assert ia.lib.ibu_labels_set(ctx._c, lb._c, None, None, 0, C.byref(skipped), None) == 0 and skipped.value == 0
            assert ia.lib.ibu_labels_get(ctx._c, lb._c, None, 0, 9, None, None) == 0
            assert lb.set([], []) == 0 and len(lb.get([])) == 0
            assert (lb.get(u) == lb_np.lab).all()
            ar.check("k == 0")
    finally:
        ar.free()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ia, ctx):
    bc_len, n = 16, 1000
    wl, by_order = _case(bc_len, 1000)
    recs = by_order["shuffled"][:n]
    lib = ia.lib

    def refused(rc):
        return rc != 0 and lib.ibu_status_name(rc) == b"InvalidArg"

    other = ia.Context(0)
    ar = _arena(ia, ctx, 24 * n, n)
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, _whitelist(ia, ctx, wl[:10], bc_len) as h2, _whitelist(ia, other, wl, bc_len) as h3:
            lb, lb2, lb3 = h.labels(fill=1), h2.labels(fill=2), h3.labels(fill=3)
            d, d_cls = ar.carve(24 * n, 8), ar.carve(n, 1)
            d.upload(recs)
            d_cls.upload(np.full(n, PATTERN, np.uint8))
            hist = (C.c_uint64 * 257)(*([GARBAGE] * 257))
            ok = (ctx._c, lb._c, _p(d), n, 0, 0, 255, _p(d_cls), hist, None)

            def label(**kw):
                names = ("ctx", "lb", "recs", "n", "flags", "match", "missing", "cls", "hist", "stream")
                return lib.ibu_label_records(*[kw.get(k, v) for k, v in zip(names, ok)])

            assert refused(label(lb=lb3._c)) and refused(label(ctx=other._c))                  # labels of another context
            assert refused(label(lb=None)) and refused(label(ctx=None))
            for flags in (2, 3, 1 << 31):
                assert refused(label(flags=flags)), flags                                      # an unknown flag
            assert refused(label(match=256)) and refused(label(match=256, flags=1)) and refused(label(match=1 << 31, flags=1))
            assert refused(label(missing=256))
            assert refused(label(recs=None)) and refused(label(recs=C.c_void_p(d.ptr + 4)))    # a misaligned records pointer
            assert refused(label(n=1 << 40))
            assert refused(label(match=256, n=0)), "checked whatever n is"
            ar.check("refused calls")
            assert (d_cls.download(np.uint8, n) == PATTERN).all() and list(hist) == [GARBAGE] * 257, "a refused call touches nothing"
            assert d.download(count=24 * n).tobytes() == recs.tobytes()
            # create, set and get
            h4 = C.c_void_p()
            assert refused(lib.ibu_labels_create(ctx._c, h3._c, 255, None, C.byref(h4))) and not h4.value   # a whitelist of another context
            assert refused(lib.ibu_labels_create(other._c, h._c, 255, None, C.byref(h4))) and not h4.value
            assert refused(lib.ibu_labels_create(ctx._c, None, 255, None, C.byref(h4)))
            assert refused(lib.ibu_labels_create(ctx._c, h._c, 256, None, C.byref(h4))) and not h4.value    # fill above 255
            assert refused(lib.ibu_labels_set(ctx._c, lb3._c, _p(d), _p(d_cls), 1, None, None))
            assert refused(lib.ibu_labels_set(ctx._c, lb._c, C.c_void_p(d.ptr + 4), _p(d_cls), 1, None, None))
            assert refused(lib.ibu_labels_set(ctx._c, lb._c, _p(d), None, 1, None, None))
            assert refused(lib.ibu_labels_get(ctx._c, lb3._c, _p(d), 1, 0, _p(d_cls), None))
            assert refused(lib.ibu_labels_get(ctx._c, lb._c, _p(d), 1, 256, _p(d_cls), None))
            assert refused(lib.ibu_labels_get(ctx._c, lb._c, _p(d), 1, 0, None, None))
            ar.check("refused set and get")
            assert (d_cls.download(np.uint8, n) == PATTERN).all() and (lb.get(np.unique(wl)) == 1).all()
            # n == 0 is OK and touches nothing: hist is all zero
            assert label(n=0) == 0 and list(hist) == [0] * 257
            assert label(n=0, recs=None, cls=None) == 0
            assert ctx.label_records(lb, d, 0, hist=True).tolist() == [0] * 257
            # Labels act through the whitelist they were created on — no call takes labels and a whitelist together, so labels of
            # ANOTHER whitelist are no refusal: they label by that whitelist, here its ten entries, every one with label 2.
            assert label(lb=lb2._c) == 0
            ar.check("labels of the smaller whitelist")
            want_cls, want_hist = lnp.label_records(lnp.Labels(wl[:10], bc_len, 2), recs)
            assert d_cls.download(np.uint8, n).tobytes() == want_cls.tobytes() and np.array(hist, dtype=np.uint64).tobytes() == want_hist.tobytes()
            for x in (lb, lb2, lb3):
                x.close()
            lb.close()                                                                         # twice is harmless
    finally:
        ar.free()
        other.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_hashtag_assignment_splits_the_expression_library(ia, ctx):
    """assign_features on the hashtag records -> labels_from_assignment -> label_records on the gene-expression records of the same
    cells: the histogram is the reads per sample, and match mode with select_records extracts every sample — twelve hashtags, so
    labels pass 7, which select_records alone could never keep."""
    bc_len, n_cells, n_tags = 16, 300, 12
    rng = np.random.default_rng(0x1AB0500)
    cells = lnp.whitelist(rng, bc_len, n_cells)
    hashtags = [3, 5, 8, 13, 21, 22, 23, 30, 31, 34, 38, 39]                 # their numbers in the hashtag library's feature list
    # the hashtag library: cells 0..279 (280..299 have no hashtag record at all).  A clean cell has 30 molecules of its hashtag and 3 of
    # another; cells 240..259 are mixed (two hashtags, 15 molecules each); cells 260..279 have two molecules only (below min_value)
    rows = []
    for c in range(280):
        tag = c % n_tags
        other = (tag + 1 + c % 5) % n_tags
        for t, k in ((tag, 30), (other, 3)) if c < 240 else ((tag, 15), (other, 15)) if c < 260 else ((tag, 2),):
            rows += [(cells[c], u, hashtags[t]) for u in range(k) for _ in range(1 + (u + c) % 2)]
    hto = np.array(rows, dtype=cnp.REC)[rng.permutation(len(rows))]
    # the gene-expression library: cells 20..299 (0..19 occur in the hashtag library only) and 2000 reads of barcodes that are no cell
    n_gex = 20_000
    gex = np.zeros(n_gex, cnp.REC)
    gex["barcode"] = np.concatenate([cells[rng.integers(20, n_cells, n_gex - 2000)], lnp.outsiders(rng, cells, bc_len, 2000)])[rng.permutation(n_gex)]
    gex["barcode"] = wnp.with_junk(rng, gex["barcode"], bc_len)
    gex["umi"], gex["index"] = rng.integers(0, 1 << 24, n_gex, dtype=np.uint64), rng.integers(0, 2000, n_gex, dtype=np.uint64)
    # numpy: the assignment, then the label of every expression read
    (b, i, reads, umis), _ = cnp.count_matrix(hto)
    top = rt.row_top(b, i, umis)
    row_cls, counts = rt.assign(top[1], top[2], top[3], 3, 2, 3)
    assert counts["assigned"] == 240 and counts["mixed"] == 20 and counts["none"] == 20
    row_bc = b[rt.row_starts(b)]
    lab = np.where(row_cls == rt.ROW_ASSIGNED, [hashtags.index(int(t)) if int(t) in hashtags else 0 for t in top[0]],
                   np.where(row_cls == rt.ROW_MIXED, 254, 253)).astype(np.uint8)
    lb_np = lnp.Labels(row_bc, bc_len)
    assert lnp.set_labels(lb_np, row_bc, lab) == 0
    cls_np, hist_np = lnp.label_records(lb_np, gex)
    assert (hist_np[:n_tags] > 0).all() and hist_np[254] > 0 and hist_np[253] > 0 and hist_np[256] >= 2000
    assert int(hist_np[:n_tags].sum() + hist_np[254] + hist_np[253] + hist_np[256]) == n_gex
    # the device
    d_hto, tmp, d_gex, d_cls = ctx.upload(hto), ctx.alloc(24 * len(hto)), ctx.upload(gex), ctx.alloc(n_gex)
    ctx.count_matrix(d_hto, tmp, len(hto), leave_swapped=True)
    d_keys, row_top, d_row_cls, got_counts = ctx.assign_features(d_hto, len(hto), min_value=3, min_share=(2, 3))
    assert got_counts == ia.AssignCounts(**counts)
    with pytest.raises(ValueError):
        ctx.labels_from_assignment(d_keys, row_top, d_row_cls, list(range(254)), bc_len)
    wl, lb = ctx.labels_from_assignment(d_keys, row_top, d_row_cls, hashtags, bc_len)
    try:
        assert wl.n_distinct == len(row_bc) == 280 and (lb.get(row_bc) == lab).all()
        hist = ctx.label_records(lb, d_gex, n_gex, d_class=d_cls, hist=True)
        assert hist.tobytes() == hist_np.tobytes() and d_cls.download(np.uint8, n_gex).tobytes() == cls_np.tobytes()
        assert ctx.label_records(lb, d_gex, n_gex, hist=True).tobytes() == hist_np.tobytes()   # the "reads per sample" query
        kept_total = 0
        for sample in list(range(n_tags)) + [254, 253]:
            assert ctx.label_records(lb, d_gex, n_gex, d_class=d_cls, match=sample) is None
            out, k = ctx.select_records(d_gex, d_cls, n_gex, 1 << ia.LABEL_IS)
            want = gex[cls_np == sample]
            assert k == len(want) == hist_np[sample] and out.download(cnp.REC, k).tobytes() == want.tobytes(), sample
            out.free()
            kept_total += k
        assert kept_total + int(hist[256]) == n_gex
        assert d_gex.download(cnp.REC, n_gex).tobytes() == gex.tobytes()
    finally:
        lb.close()
        wl.close()
        row_top.free()
        for x in (d_hto, tmp, d_gex, d_cls, d_keys, d_row_cls):
            x.free()


def test_count_file_example_keeps_one_label(ia, tmp_path):
    """count_file --labels=FILE --keep-label=L --label-hist: the reads per label and the matrix of one sample of a small file."""
    import os
    import subprocess
    from ibu_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len, n = 16, 5000
    rng = np.random.default_rng(0x1AB0600)
    cells = lnp.whitelist(rng, bc_len, 60)
    labs = (np.arange(60) % 12).astype(np.uint8)
    recs = np.zeros(n, cnp.REC)
    recs["barcode"] = np.concatenate([cells[rng.integers(0, 60, n - 500)], lnp.outsiders(rng, cells, bc_len, 500)])[rng.permutation(n)]
    recs["umi"], recs["index"] = rng.integers(0, 40, n, dtype=np.uint64), rng.integers(0, 30, n, dtype=np.uint64)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()

    def text(code):
        return "".join("ACGT"[(int(code) >> (2 * i)) & 3] for i in range(bc_len))   # base i at bits [2i, 2i+1]

    (tmp_path / "labels.txt").write_text("".join(f"{text(c)} {int(v)}\n" for c, v in zip(cells, labs)))
    lb_np = lnp.Labels(cells, bc_len)
    lnp.set_labels(lb_np, cells, labs)
    cls_np, hist_np = lnp.label_records(lb_np, recs)
    sample = 9
    (b, i, reads, umis), _ = cnp.count_matrix(recs[cls_np == sample])
    r = subprocess.run([str(exe), f"--labels={tmp_path / 'labels.txt'}", f"--keep-label={sample}", "--label-hist", str(tmp_path / "in.ibu")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [ln for ln in lines if not ln.startswith("#")] == [f"{text(bb)}\t{ii}\t{uu}\t{rr}" for bb, ii, rr, uu in zip(b.tolist(), i.tolist(), reads.tolist(), umis.tolist())]
    assert [ln for ln in lines if ln.startswith("#label")] == [f"#label\t{k}\t{int(hist_np[k])}" for k in range(12)] + [f"#label\t-\t{int(hist_np[256])}"]
    assert f"{n} records: label {sample}; kept {int(hist_np[sample])}" in r.stderr and hist_np[sample] > 0 and hist_np[256] == 500
    r = subprocess.run([str(exe), "--keep-label=9", str(tmp_path / "in.ibu")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--labels=FILE" in r.stderr
