"""What the C ABI refuses, and in which words: one table of refused calls through the raw ctypes `lib`, each with its status name,
its detail words a / b and its exact message (ibu_last_error).  Every call works on one device buffer of 64 records and stays inside
it, so that a call whose check went missing would compute on valid memory.  NULL pointers and counts of 2^40 and more are the host
test's (tests/test_api_checks.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
ALIGNED = "{} must be non-NULL and 8-byte aligned"


@pytest.fixture(scope="module")
def env(oracle):
    import ibu_amd as ia
    e = type("Env", (), {})()
    e.ia, e.lib = ia, ia.lib
    e.ctx, e.other = ia.Context(0), ia.Context(0)
    recs = oracle.sort_records(oracle.generate(0x1B00020, 0, N, 2, 3))
    e.barcodes = len(np.unique(recs["barcode"]))
    e.pairs = len(np.unique(recs[["barcode", "umi"]]))
    e.buf = e.ctx.upload(recs)
    e.tmp, e.out = e.ctx.alloc(24 * N), e.ctx.alloc(24 * N)
    e.cls = e.ctx.upload(np.zeros(N, np.uint8))            # every record of class 0: a keep mask of 1 keeps all 64
    e.cols = [e.ctx.alloc(8 * N) for _ in range(6)]
    words = ["AC", "GT", "TT"]
    e.wl, e.wl_other = ia.Whitelist.from_ascii(e.ctx, words), ia.Whitelist.from_ascii(e.other, words)
    e.ab = e.wl.abundance()
    e.size = C.c_size_t(12345)
    e.size2 = C.c_size_t(12345)
    yield e
    e.ctx.synchronize()
    e.ab.close()
    e.wl.close()
    e.wl_other.close()
    for b in [e.buf, e.tmp, e.out, e.cls] + e.cols:
        b.free()
    e.other.close()
    e.ctx.close()


def _capacity(what, cap, need, see):
    return f"output capacity {cap} is smaller than the {need} {what} (see *{see})"


def _saturation(e, k):
    ts = (C.c_uint64 * 33)(*range(33))
    pts = (e.ia._lib.CSaturationPoint * 33)()
    return e.lib.ibu_saturation_curve(e.ctx._c, e.buf.ptr, N, 0, 1, ts, k, pts, None)


# name -> (the call, a, b, message behind "Invalid argument: ", the value the call leaves in e.size or None)
ROWS = {
    "sort_misaligned": (lambda e: e.lib.ibu_sort_records(e.ctx._c, e.buf.ptr + 4, e.tmp.ptr, 2, None),    # (one record is sorted: n = 2)
                        0, 0, lambda e: ALIGNED.format("d_records / d_tmp"), None),
    "reduce_misaligned": (lambda e: e.lib.ibu_reduce(e.ctx._c, e.buf.ptr + 4, 1, None), 0, 0, lambda e: ALIGNED.format("d_records"), None),
    "correct_misaligned": (lambda e: e.lib.ibu_correct_barcodes(e.ctx._c, e.wl._c, e.buf.ptr + 4, 1, 1, e.cls.ptr, None, None),
                           0, 0, lambda e: ALIGNED.format("d_records"), None),
    "select_misaligned": (lambda e: e.lib.ibu_select_records(e.ctx._c, e.buf.ptr + 4, e.cls.ptr, 1, 1, e.out.ptr, 1, C.byref(e.size), None),
                          0, 0, lambda e: ALIGNED.format("d_records"), lambda e: 0),
    "pair_counts_misaligned": (lambda e: e.lib.ibu_pair_counts(e.ctx._c, e.buf.ptr + 4, 1, *[c.ptr for c in e.cols[:4]], 1, C.byref(e.size),
                                                               C.byref(e.size2), None),
                               0, 0, lambda e: ALIGNED.format("d_sorted_records"), lambda e: 0),
    "call_cells_misaligned": (lambda e: e.lib.ibu_call_cells(e.ctx._c, e.buf.ptr + 4, 1, e.ia.CELLS_MIN, 1, 0, e.cls.ptr, None, None),
                              0, 0, lambda e: ALIGNED.format("d_sorted_records"), None),
    # records 0..31 in, d_out at record 31 with room for 32: one record shared
    "select_out_overlaps": (lambda e: e.lib.ibu_select_records(e.ctx._c, e.buf.ptr, e.cls.ptr, 32, 1, e.buf.ptr + 24 * 31, 32, C.byref(e.size), None),
                            0, 0, lambda e: "d_out overlaps d_records", lambda e: 0),
    "merge_runs_tmp_overlaps": (lambda e: e.lib.ibu_merge_sorted_runs(e.ctx._c, e.buf.ptr, e.buf.ptr + 24 * 31, (C.c_size_t * 2)(16, 16), 2, None),
                                0, 0, lambda e: "d_tmp overlaps d_records", None),
    "barcode_counts_capacity": (lambda e: e.lib.ibu_barcode_counts(e.ctx._c, e.buf.ptr, N, *[c.ptr for c in e.cols[:3]], e.barcodes - 1,
                                                                   C.byref(e.size), C.byref(e.size2), None),
                                0, 0, lambda e: "output capacity is smaller than the number of distinct barcodes (see *n_barcodes)",
                                lambda e: e.barcodes),
    "pair_counts_capacity": (lambda e: e.lib.ibu_pair_counts(e.ctx._c, e.buf.ptr, N, *[c.ptr for c in e.cols[:4]], e.pairs - 1, C.byref(e.size),
                                                             C.byref(e.size2), None),
                             lambda e: e.pairs, lambda e: e.pairs - 1, lambda e: _capacity("entries", e.pairs - 1, e.pairs, "n_pairs"),
                             lambda e: e.pairs),
    "select_capacity": (lambda e: e.lib.ibu_select_records(e.ctx._c, e.buf.ptr, e.cls.ptr, N, 1, e.out.ptr, N - 1, C.byref(e.size), None),
                        N, N - 1, lambda e: _capacity("records kept", N - 1, N, "n_out"), lambda e: N),
    "barcode_metrics_capacity": (lambda e: e.lib.ibu_barcode_metrics(e.ctx._c, e.buf.ptr, N, None, 0, 1, *[c.ptr for c in e.cols], e.barcodes - 1,
                                                                     C.byref(e.size), None),
                                 lambda e: e.barcodes, lambda e: e.barcodes - 1,
                                 lambda e: _capacity("barcodes", e.barcodes - 1, e.barcodes, "n_barcodes"), lambda e: e.barcodes),
    "correct_foreign_whitelist": (lambda e: e.lib.ibu_correct_barcodes(e.ctx._c, e.wl_other._c, e.buf.ptr, N, 1, e.cls.ptr, None, None),
                                  0, 0, lambda e: "the whitelist was created on another context", None),
    "resolve_foreign_whitelist": (lambda e: e.lib.ibu_resolve_barcodes(e.ctx._c, e.wl_other._c, e.ab._c, e.buf.ptr, N, 2, 3, e.cls.ptr, None, None),
                                  0, 0, lambda e: "the whitelist was created on another context", None),
    "resolve_share_one_half": (lambda e: e.lib.ibu_resolve_barcodes(e.ctx._c, e.wl._c, e.ab._c, e.buf.ptr, N, 1, 2, e.cls.ptr, None, None),
                               0, 0, lambda e: "the share num / den must satisfy 1 <= num <= den < 2^24 and 2 * num > den", None),
    "saturation_no_points": (lambda e: _saturation(e, 0), 0, 0, lambda e: "k must be 1..32", None),
    "saturation_33_points": (lambda e: _saturation(e, 33), 0, 0, lambda e: "k must be 1..32", None),
}


@pytest.mark.parametrize("name", list(ROWS))
def test_refused_call_says_exactly_this(env, name):
    call, a, b, message, left = ROWS[name]
    env.size.value = env.size2.value = 12345
    rc = call(env)
    d = env.ia._lib.CErrorDetail()
    env.lib.ibu_last_error(C.byref(d))
    assert env.lib.ibu_status_name(rc).decode() == "InvalidArg" and d.code == rc
    assert d.message.decode() == "Invalid argument: " + message(env)
    assert (d.a, d.b) == (a(env) if callable(a) else a, b(env) if callable(b) else b)
    if left is not None:
        assert env.size.value == left(env)
