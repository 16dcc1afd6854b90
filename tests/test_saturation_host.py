"""Read subsampling and the saturation curve (ibu_subsample_class, ibu_saturation_curve) — what can be checked without a GPU: the
numpy statement of the semantics (tests/saturation_np.py) against a brute force over the runs and against cases a reader can check
by eye, the entry points in every layer of the ABI, the argument errors that need no device, the loud failure on a box without one,
the example program, and the layout the benchmark tool lays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import count_np
from tests import saturation_np as snp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_subsample_class", "ibu_saturation_curve")
GARBAGE = 0x5A5A5A5A5A5A5A5A


def _recs(rows):
    return np.array(rows, snp.REC).reshape(-1)


def _random_recs(rng, case):
    """n <= 200 records with long and short runs; every third case permuted (the runs of unsorted input)."""
    n = int(rng.integers(1, 201))
    nb, nu = int(rng.integers(1, 8)), int(rng.integers(1, 6))
    r = np.zeros(n, snp.REC)
    r["barcode"], r["umi"], r["index"] = rng.integers(0, nb, n), rng.integers(0, nu, n), rng.integers(0, 3, n)
    if case % 4 == 3:                                              # one long run and a few short ones
        r["barcode"][: n - n // 8] = 99
        r["umi"][: n // 2] = 7
    r = count_np.sort_records(r)
    if case % 3 == 2:
        r = r[rng.permutation(n)]
    return r


def _thresholds(rng, uu):
    """0, all ones, duplicates, and u-values themselves: t = u(row) (not kept: the inequality is strict) and u(row) + 1 (kept)."""
    rows = rng.integers(0, len(uu), 3)
    ts = [0, snp.ONES, 1 << 63, 1 << 63, int(rng.integers(0, 1 << 63)) * 2]
    for r in rows:
        ts += [int(uu[r]), min(int(uu[r]) + 1, snp.ONES)]
    return sorted(ts)


def test_numpy_statement_equals_brute_force():
    rng = np.random.default_rng(0x32100)
    strict = 0
    for case in range(300):
        recs = _random_recs(rng, case)
        seed, first_row = int(rng.integers(0, 1 << 63)), (0, 1, (1 << 40) + 3, snp.ONES)[case % 4]
        uu = snp.u(seed, first_row, len(recs))
        ts = _thresholds(rng, uu)
        got, want = snp.saturation_curve(recs, seed, first_row, ts), snp.brute_force(recs, seed, first_row, ts)
        assert got == want, (case, got, want)
        cls, k = snp.subsample_class(len(recs), seed, first_row, ts[3])
        assert cls.dtype == np.uint8 and k == int((cls == snp.KEPT).sum()) == got[3][1]
        strict += sum(b[1] == a[1] + 1 for a, b in zip(got, got[1:]) if b[0] == a[0] + 1)
    assert strict > 600, "u(row) and u(row) + 1 differ by exactly the read of that row"


def test_pinned_values_and_hand_written_cases():
    assert snp.splitmix64(0) == 0xE220A8397B1DCDAF
    assert int(snp.u(0, 0, 1)[0]) == 0xA706DD2F4D197E6F == snp.splitmix64(snp.splitmix64(0))
    assert snp.u(0, 5, 3).tolist() == snp.u(0, 0, 8)[5:].tolist(), "first_row: the pieces of a larger array hash as the whole would"
    assert snp.u(0, snp.ONES, 2).tolist()[1] == int(snp.u(0, 0, 1)[0]), "the sums wrap"
    # seed 0: u = 0xA706.., 0x2A98.., 0x8287.., 0xF9BF.. for rows 0 .. 3: by size row 1, row 2, row 0, row 3
    uu = [int(x) for x in snp.u(0, 0, 4)]
    assert [x >> 48 for x in uu] == [0xA706, 0x2A98, 0x8287, 0xF9BF]
    recs = _recs([(5, 1, 0), (5, 1, 1), (5, 2, 0), (6, 1, 0)])       # barcodes {5: rows 0-2, 6: row 3}; molecules {0-1}, {2}, {3}
    T = lambda top: top << 60
    ts = [0, T(1), T(3), T(9), T(0xB), T(0xF), snp.ONES]
    curve = snp.saturation_curve(recs, 0, 0, ts)
    assert curve == snp.brute_force(recs, 0, 0, ts) and [c[0] for c in curve] == ts
    assert [c[1:] for c in curve] == [(0, 0, 0),                  # t = 0 keeps nothing
                                      (0, 0, 0),                  # every u is above 0x1000..
                                      (1, 1, 1),                  # row 1: barcode 5, molecule (5, 1)
                                      (2, 1, 2),                  # + row 2: molecule (5, 2), no new barcode
                                      (3, 1, 2),                  # + row 0: a second read of molecule (5, 1)
                                      (3, 1, 2),                  # row 3 is 0xF9BF.., not below 0xF000..
                                      (4, 2, 3)]                  # all ones: row 3 too, barcode 6
    assert snp.subsample_class(4, 0, 0, T(9))[0].tolist() == [1, 0, 0, 1]
    assert snp.subsample_class(4, 0, 0, uu[1])[1] == 0 and snp.subsample_class(4, 0, 0, uu[1] + 1)[1] == 1, "strictly below"
    assert snp.subsample_class(4, 0, 0, 0)[1] == 0 and snp.subsample_class(4, 0, 0, snp.ONES)[1] == 4
    # identical records are different reads; an interrupted run is two runs
    same = _recs([(1, 1, 1)] * 4)
    assert snp.saturation_curve(same, 0, 0, [T(9)]) == [(T(9), 2, 1, 1)]
    back = _recs([(5, 1, 0), (6, 1, 0), (5, 1, 0)])
    assert snp.saturation_curve(back, 0, 0, [snp.ONES]) == [(snp.ONES, 3, 3, 3)]
    assert snp.saturation_curve(np.zeros(0, snp.REC), 3, 4, [0, 7, snp.ONES]) == [(0, 0, 0, 0), (7, 0, 0, 0), (snp.ONES, 0, 0, 0)]
    assert snp.brute_force(np.zeros(0, snp.REC), 3, 4, [7]) == [(7, 0, 0, 0)]


def test_nesting_order_and_the_full_depth():
    rng = np.random.default_rng(0x32200)
    for case in range(60):
        recs = _random_recs(rng, case)
        n = len(recs)
        ts = sorted(2 * int(x) for x in rng.integers(0, 1 << 63, 6)) + [snp.ONES]
        curve = snp.saturation_curve(recs, case, 0, ts)
        for a, b in zip(curve, curve[1:]):
            assert all(x <= y for x, y in zip(a[1:], b[1:])), "a non-decreasing threshold list gives non-decreasing points"
        assert all(c[2] <= c[3] <= c[1] for c in curve), "barcodes <= molecules <= reads"
        pairs = count_np.pair_counts(recs)
        w = count_np._words(recs)
        barcodes = 1 + int((w[1:, 0] != w[:-1, 0]).sum())
        assert curve[-1][1:] == (n, barcodes, len(pairs[0]))
        classes = [snp.subsample_class(n, case, 0, t)[0] for t in ts]
        for a, b in zip(classes, classes[1:]):
            assert not ((a == snp.KEPT) & (b == snp.DROPPED)).any(), "a read kept at t is kept at every larger t"


def test_sample_threshold_is_exact():
    import ibu_amd
    from fractions import Fraction
    f = ibu_amd.sample_threshold
    assert f(0) == 0 and f(0.5) == 1 << 63 and f(1) == f(1.5) == f(7) == snp.ONES and f(1 / 4096) == 1 << 52
    assert f(Fraction(1, 3)) == (1 << 64) // 3 and f(0.1) == int(Fraction(0.1) * (1 << 64)) == snp.sample_threshold(0.1)
    assert f(float(np.nextafter(1.0, 0.0))) == (1 << 64) - (1 << 11), "the largest double below 1"
    for bad in (-0.5, float("nan"), -1):
        with pytest.raises(ValueError):
            f(bad)


def test_entry_points_exist_in_every_layer():
    import ibu_amd
    from ibu_amd import _lib
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    so = C.CDLL(_lib.SO_PATH)
    for name, arity in zip(NAMES, (8, 9)):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in ibu_hip.h"
        assert hasattr(so, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity
        assert re.search(r"pub fn %s\s*\(" % name, ffi)
        short = name[4:]
        assert re.search(r"pub fn %s\s*\(" % short, lib_rs) and re.search(r"\b%s\s*\(" % short, hpp) and hasattr(ibu_amd.Context, short)
        # the arguments of the declaration, in order, are the Rust extern's
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        c_args = [re.search(r"(\w+)\s*$", a.strip()).group(1) for a in decl.split(",")]
        rust = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, ffi, flags=re.S).group(1)
        assert c_args == [a.split(":")[0].strip() for a in rust.split(",")] and len(c_args) == arity
    for name, value in (("IBU_SAMPLE_KEPT", "0"), ("IBU_SAMPLE_DROPPED", "1"), ("IBU_SATURATION_MAX_POINTS", "32u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert (ibu_amd.SAMPLE_KEPT, ibu_amd.SAMPLE_DROPPED, ibu_amd.SATURATION_MAX_POINTS) == (0, 1, 32) == (snp.KEPT, snp.DROPPED, snp.MAX_POINTS)
    assert ibu_amd.SaturationPoint._fields == snp.FIELDS
    assert "pub struct ibu_saturation_point_t" in ffi and "SaturationPoint" in hpp
    assert C.sizeof(_lib.CSaturationPoint) == 32 and tuple(f for f, _ in _lib.CSaturationPoint._fields_) == snp.FIELDS
    fields = re.search(r"typedef struct ibu_saturation_point \{(.*?)\}", code, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == snp.FIELDS
    rust_fields = re.search(r"pub struct ibu_saturation_point_t \{(.*?)\}", ffi, flags=re.S).group(1)
    assert tuple(re.findall(r"pub (\w+): u64", rust_fields)) == snp.FIELDS
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "a new entry point changes no signature"


def test_kernels_are_in_the_code_object_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = kernel_resources.all_kernels(_lib.SO_PATH)
    for k in ("ibu_k_saturation_walk", "ibu_k_saturation_sum", "ibu_k_saturation_stitch", "ibu_k_saturation_points", "ibu_k_subsample"):
        assert k in ks, k
        assert ks[k].get("private_segment_fixed_size", 0) == 0 and not ks[k].get("uses_dynamic_stack", 0), (k, ks[k])


def test_python_wrapper_refuses_before_the_library_is_called():
    """The context is never looked at."""
    import ibu_amd
    c = object.__new__(ibu_amd.Context)
    sub, curve = ibu_amd.Context.subsample_class, ibu_amd.Context.saturation_curve
    for kw in ({}, {"fraction": 0.5, "threshold": 7}):
        with pytest.raises(ValueError, match="exactly one of"):
            sub(c, 1, None, **kw)
    for kw in ({"fraction": -1}, {"fraction": float("nan")}, {"threshold": -1}, {"threshold": 1 << 64}, {"fraction": 0.5, "seed": -1},
               {"fraction": 0.5, "seed": 1 << 64}, {"fraction": 0.5, "first_row": 1 << 64}, {"fraction": 0.5, "d_class": False, "count": False}):
        with pytest.raises(ValueError):
            sub(c, 1, **kw)
    for kw in ({}, {"fractions": [0.5], "thresholds": [7]}):
        with pytest.raises(ValueError, match="exactly one of"):
            curve(c, None, 1, **kw)
    for kw in ({"fractions": []}, {"fractions": [0.1] * 33}, {"thresholds": [2, 1]}, {"fractions": [0.5, 0.25]}, {"fractions": [-0.5]},
               {"thresholds": [1 << 64]}, {"thresholds": [-1]}, {"fractions": [0.5], "seed": -1}, {"fractions": [0.5], "first_row": -1}):
        with pytest.raises(ValueError):
            curve(c, None, 1, **kw)


def test_both_calls_fail_loudly_without_gpu():
    """A NULL context is an error whatever the other arguments say, never a host computation, and leaves the outputs alone; without
    a device the Python Context cannot exist."""
    import ibu_amd
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    sub, curve = so.ibu_subsample_class, so.ibu_saturation_curve
    sub.restype, sub.argtypes = _lib.SIGNATURES[NAMES[0]]
    curve.restype, curve.argtypes = _lib.SIGNATURES[NAMES[1]]
    k = C.c_size_t(GARBAGE)
    for n, t, with_k in ((1, 7, True), (0, 0, True), (1 << 40, 7, True), (1, snp.ONES, False), (0, 0, False)):
        assert sub(None, n, 0, 0, t, None, C.byref(k) if with_k else None, None) != 0
        assert k.value == GARBAGE
    pts = (_lib.CSaturationPoint * 33)(*[_lib.CSaturationPoint(*[GARBAGE] * 4) for _ in range(33)])
    up, down = (C.c_uint64 * 33)(*range(33)), (C.c_uint64 * 2)(2, 1)
    for n, ts, kk, p in ((1, up, 3, pts), (0, up, 3, pts), (1, up, 0, pts), (1, up, 33, pts), (1, down, 2, pts), (1, None, 1, pts), (1, up, 1, None),
                         (1 << 40, up, 1, pts), (0, up, 32, pts)):
        assert curve(None, None, n, 0, 0, ts, kk, p, None) != 0
        assert all(getattr(q, f) == GARBAGE for q in pts for f in snp.FIELDS), "a refused call leaves the points alone"
    if ibu_amd.device_count() > 0:
        return
    for call in (lambda c: c.subsample_class(1, fraction=0.5), lambda c: c.saturation_curve(None, 1, fractions=[0.5, 1])):
        with pytest.raises(ibu_amd.IbuError) as ei:
            call(ibu_amd.Context(0))
        assert ei.value.kind == "NoDevice"


def test_count_file_example_compiles_with_the_two_options(tmp_path):
    from ibu_amd import _lib
    src = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    assert "[--subsample=F[:seed]] [--saturation=K]" in src and "saturation_curve" in src and "subsample_class" in src
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    malformed = ["--saturation=0", "--saturation=33", "--saturation=", "--saturation", "--saturation=ten", "--saturation=5x", "--saturation=-1",
                 "--subsample=", "--subsample", "--subsample=-0.5", "--subsample=nan", "--subsample=half", "--subsample=0.5:", "--subsample=0.5:x",
                 "--subsample=0.5:7:1", "--subsample=0.5x"]
    for args in [["--saturation=10"], ["--subsample=0.5:7", "--saturation=10"]] + [[m, "x.ibu"] for m in malformed]:
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.returncode == 2 and "usage: count_file" in r.stderr and "--saturation=K" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("n,rpm", [(2_003, 4), (10_007, 4), (123_457, 4), (123_456, 3), (250_001, 5)])
def test_the_benchmark_lays_exactly_n_records(n, rpm):
    """tools/aggbench.py --saturation checks the library against the layout it laid: replayed here on the CPU, the rows are sorted
    and the numpy statement finds in them, at full depth, n reads and exactly the barcodes and molecules the layout says."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import aggbench
    bc, um, ix = aggbench.molecule_fill(torch, torch.arange(n, dtype=torch.int64), rpm, int(0.05 * (1 << 20)))
    recs = np.zeros(n, snp.REC)
    recs["barcode"], recs["umi"], recs["index"] = bc.numpy().astype(np.uint64), um.numpy().astype(np.uint64), ix.numpy().astype(np.uint64)
    assert recs.tobytes() == count_np.sort_records(recs).tobytes()
    barcodes, molecules = aggbench.molecule_layout(n, rpm)
    half, full = snp.saturation_curve(recs, 0x1B0000C, 0, [1 << 63, snp.ONES])
    assert full[1:] == (n, barcodes, molecules) and molecules == len(count_np.pair_counts(recs)[0])
    assert abs(half[1] - n / 2) < 4 * (n ** 0.5) and half[3] < molecules and half[2] == barcodes
