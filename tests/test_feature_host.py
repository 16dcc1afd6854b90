"""Per-feature metrics and the feature filter (ibu_feature_metrics, ibu_filter_features) — what can be checked without a GPU: the
numpy statement of the semantics (tests/feature_np.py) against its brute-force twin and against cases a reader can check by eye, the
entry points in every layer of the ABI, the kernels' resources, the argument errors that need no device, the loud failure on a box
without one, and the example program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import feature_np as fnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_feature_metrics", "ibu_filter_features")
GARBAGE = 0x5A5A5A5A5A5A5A5A
# values on either side of the table sizes the tests use (1, 4, 64, 65) and two above 2^32 whose low bits name a feature
PALETTE = np.array([0, 1, 2, 3, 4, 63, 64, 65, (1 << 32) + 1, (1 << 32) + 63], np.uint64)
HAND = [(1, 0, 5), (1, 0, 5), (1, 0, 6), (1, 2, 5), (2, 0, 5), (2, 4, 1), (2, (1 << 32) + 2, 1)]


def _recs(rows):
    return np.array(rows, fnp.REC)


def _random_records(rng, n):
    r = np.zeros(n, fnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    w[:, 0] = np.sort(rng.integers(0, max(n // 4, 1) + 1, n)).astype(np.uint64)
    w[:, 1] = PALETTE[rng.integers(0, len(PALETTE), n) // 2 * 2 % len(PALETTE)]
    w[:, 2] = PALETTE[rng.integers(0, len(PALETTE), n)]
    if rng.integers(0, 3):                                       # mostly sorted, sometimes the runs as they stand
        r = r[np.lexsort((w[:, 2], w[:, 1], w[:, 0]))]
    return r


def test_numpy_statement_equals_brute_force():
    rng = np.random.default_rng(0x51100)
    seen = set()
    for case in range(300):
        n = int(rng.integers(0, 120))
        recs = _random_records(rng, n)
        nf = int(rng.choice([1, 4, 64, 65, 70]))
        word = 1 + (case & 1)
        table, totals = fnp.feature_metrics(recs, nf, word)
        lim = fnp.limits(min_reads=int(rng.integers(0, 3)), max_reads=int(rng.integers(0, 12)), min_umis=int(rng.integers(0, 3)),
                         max_umis=int(rng.integers(0, 8)))
        if word == 1:
            lim.update(min_cells=int(rng.integers(0, 3)), max_cells=int(rng.integers(0, 5)))
        btable, btotals, (bv, bcls, btot) = fnp.brute_force(recs, nf, word, lim)
        for col, want in zip(table, btable):
            assert (col is None and want is None) or (col.dtype == np.uint64 and col.tolist() == want), case
        assert totals == btotals and totals[0] + totals[3] == n, (case, totals, btotals)
        assert (table[2] is None) == (word == 2) and (word == 1 or totals[2] == 0)
        v, cls, tot = fnp.filter_features(recs, nf, word, table, lim)
        assert v.dtype == cls.dtype == np.uint8 and v.tolist() == bv.tolist() and cls.tolist() == bcls.tolist() and tot == btot, case
        assert sum(tot["reads_by_class"]) == n and sum(tot["features_by_class"]) == nf
        seen |= set(cls.tolist())
        # accumulating two halves cut where a barcode begins is one call
        cuts = np.flatnonzero(recs["barcode"][1:] != recs["barcode"][:-1]) + 1
        if len(cuts):
            k = int(cuts[len(cuts) // 2])
            first, t1 = fnp.feature_metrics(recs[:k], nf, word)
            both, t2 = fnp.feature_metrics(recs[k:], nf, word, into=first)
            assert all((a is None and b is None) or a.tolist() == b.tolist() for a, b in zip(both, table)), case
            assert tuple(a + b for a, b in zip(t1, t2)) == totals
    assert seen == {0, 1, 2, 3}


def test_hand_written_cases():
    recs = _recs(HAND)
    (reads, umis, cells), totals = fnp.feature_metrics(recs, 4, 1)
    assert reads.tolist() == [4, 0, 1, 0] and umis.tolist() == [3, 0, 1, 0] and cells.tolist() == [2, 0, 1, 0]
    assert totals == (5, 4, 3, 2), "4 and 2^32 + 2 are out of range: the low bits do not alias"
    v, cls, tot = fnp.filter_features(recs, 4, 1, (reads, umis, cells), fnp.limits(min_cells=2))
    assert v.tolist() == [0, 1, 1, 1] and cls.tolist() == [0, 0, 0, 1, 0, 3, 3]
    assert tot == {"features_by_class": (1, 3, 0), "reads_by_class": (4, 1, 0, 2), "reserved": 0}
    assert fnp.brute_force(recs, 4, 1)[0] == ([4, 0, 1, 0], [3, 0, 1, 0], [2, 0, 1, 0])
    # the third word as the feature: reads and umis alike, no cells
    (reads2, umis2, cells2), totals2 = fnp.feature_metrics(recs, 7, 2)
    assert reads2.tolist() == [0, 2, 0, 0, 0, 4, 1] and umis2.tolist() == [0, 2, 0, 0, 0, 3, 1] and cells2 is None and totals2 == (7, 6, 0, 0)
    # a barcode head that leaves w1 unchanged begins a pair: two cells; a pair that returns counts again
    assert fnp.feature_metrics(_recs([(1, 3, 0), (2, 3, 0)]), 4, 1)[0][2].tolist() == [0, 0, 0, 2]
    again = fnp.feature_metrics(_recs([(1, 3, 0), (1, 2, 0), (1, 3, 0), (1, 3, 0)]), 4, 1)
    assert [c.tolist() for c in again[0]] == [[0, 0, 1, 3], [0, 0, 1, 2], [0, 0, 1, 2]] and again[1] == (4, 3, 3, 0)
    (r0, u0, c0), t0 = fnp.feature_metrics(np.zeros(0, fnp.REC), 3, 1)
    assert r0.tolist() == u0.tolist() == c0.tolist() == [0, 0, 0] and t0 == (0, 0, 0, 0)
    # a pair cut by the boundary between two accumulating calls counts once per call: the documented extra cell, and an extra UMI
    cut = fnp.feature_metrics(recs[2:], 4, 1, into=fnp.feature_metrics(recs[:2], 4, 1)[0])[0]
    assert cut[0].tolist() == [4, 0, 1, 0] and cut[1].tolist() == [3, 0, 1, 0] and cut[2].tolist() == [3, 0, 1, 0]
    cut = fnp.feature_metrics(recs[1:], 4, 1, into=fnp.feature_metrics(recs[:1], 4, 1)[0])[0]
    assert cut[1].tolist() == [4, 0, 1, 0] and cut[2].tolist() == [3, 0, 1, 0]

    table = (reads, umis, cells)
    verdict = lambda **kw: fnp.filter_features(recs, 4, 1, table, fnp.limits(**kw))[0].tolist()
    assert verdict() == [0, 0, 0, 0], "zeroed limits pass every feature"
    assert fnp.filter_features(recs, 4, 1, table, fnp.limits())[1].tolist() == [0, 0, 0, 0, 0, 3, 3], "but not the unknown ones"
    assert verdict(min_reads=1) == [0, 1, 0, 1], "a feature without reads is LOW as soon as a minimum is positive"
    assert verdict(min_reads=2) == [0, 1, 1, 1] and verdict(min_umis=2) == [0, 1, 1, 1] and verdict(min_cells=2) == [0, 1, 1, 1]
    assert verdict(max_reads=3) == [2, 0, 0, 0] and verdict(max_reads=4) == [0, 0, 0, 0]
    assert verdict(max_umis=2) == [2, 0, 0, 0] and verdict(max_cells=1) == [2, 0, 0, 0]
    assert verdict(min_reads=1, max_cells=1) == [2, 1, 0, 1], "LOW before HIGH"
    assert verdict(min_reads=5, max_reads=3) == [1, 1, 1, 1]
    # a column that is None needs no limit
    assert fnp.filter_features(recs, 4, 1, (reads, None, None), fnp.limits(min_reads=2))[0].tolist() == [0, 1, 1, 1]
    with pytest.raises(AssertionError):
        fnp.filter_features(recs, 4, 1, (reads, umis, None), fnp.limits(min_cells=1))


def _struct_fields(code, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, code, flags=re.S).group(1)
    return tuple(re.findall(r"\b([a-z_]+)\s*(?:\[\d+\])?\s*[,;]", body))


def test_entry_points_exist_in_every_layer(tmp_path):
    import ibu_amd
    from ibu_amd import _lib
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    so = C.CDLL(_lib.SO_PATH)
    for name, nargs in zip(NAMES, (11, 13)):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in ibu_hip.h"
        assert hasattr(so, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"pub fn %s\s*\(" % name, ffi)
        short = name[4:]
        assert re.search(r"pub fn %s\s*\(" % short, lib_rs) and re.search(r"\b%s\s*\(" % short, hpp) and hasattr(ibu_amd.Context, short)
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "new entry points change no signature"
    for name, value in (("IBU_FEATURE_PASS", "0"), ("IBU_FEATURE_LOW", "1"), ("IBU_FEATURE_HIGH", "2"), ("IBU_FEATURE_UNKNOWN", "3"),
                        ("IBU_FEATURE_ACCUMULATE", "1u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert (ibu_amd.FEATURE_PASS, ibu_amd.FEATURE_LOW, ibu_amd.FEATURE_HIGH, ibu_amd.FEATURE_UNKNOWN) == (0, 1, 2, 3) == \
        (fnp.PASS, fnp.LOW, fnp.HIGH, fnp.UNKNOWN) and ibu_amd.FEATURE_ACCUMULATE == 1
    assert ibu_amd.FeatureTable._fields[:3] == fnp.COLUMNS and ibu_amd.FeatureFilterCounts._fields == fnp.TOTALS[:-1]
    # the structs: the field order of the header in ctypes and Rust, and the sizes and offsets the header compiles to
    for cname, twin, fields in (("ibu_feature_limits", _lib.CFeatureLimits, fnp.LIMITS), ("ibu_feature_filter_counts", _lib.CFeatureFilterCounts, fnp.TOTALS)):
        assert _struct_fields(code, cname) == fields == tuple(f for f, _ in twin._fields_), cname
        rust = re.search(r"pub struct %s_t \{(.*?)\}" % cname, ffi, flags=re.S).group(1)
        assert tuple(re.findall(r"pub ([a-z_]+):", rust)) == fields, cname
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ibu_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(ibu_feature_limits_t), offsetof(ibu_feature_limits_t, min_cells),\n'
                   "         sizeof(ibu_feature_filter_counts_t), offsetof(ibu_feature_filter_counts_t, reads_by_class),\n"
                   "         offsetof(ibu_feature_filter_counts_t, reserved));\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    L, F = _lib.CFeatureLimits, _lib.CFeatureFilterCounts
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == \
        [C.sizeof(L), L.min_cells.offset, C.sizeof(F), F.reads_by_class.offset, F.reserved.offset] == [48, 32, 64, 24, 56]


def test_kernels_are_in_the_code_object_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = kernel_resources.all_kernels(_lib.SO_PATH)
    for k in ("ibu_k_feature_count", "ibu_k_feature_verdict", "ibu_k_feature_class", "ibu_k_feature_class_tail"):
        assert k in ks, k
        assert ks[k].get("private_segment_fixed_size", 0) == 0 and not ks[k].get("uses_dynamic_stack", 0), (k, ks[k])
    # no LDS beyond the walk's tiles (four waves of 3072 B) and the workgroup totals of block_accumulate
    assert ks["ibu_k_feature_count"].get("group_segment_fixed_size", 0) == 4 * 3072 + 4 * 4 * 8


def _limits_struct(lim):
    from ibu_amd import _lib
    return _lib.CFeatureLimits(*[lim[f] for f in fnp.LIMITS])


def test_refused_calls_touch_nothing_and_no_device_is_loud():
    """A NULL context is an error whatever the other arguments say, and so is every refused combination: non-zero, with `totals` and
    `counts` as they were.  Without a device the Python Context cannot exist."""
    import ibu_amd
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    metrics, filt = so.ibu_feature_metrics, so.ibu_filter_features
    metrics.restype, metrics.argtypes = _lib.SIGNATURES[NAMES[0]]
    filt.restype, filt.argtypes = _lib.SIGNATURES[NAMES[1]]
    words = (C.c_uint64 * 8)()
    at = C.addressof(words)
    # (n, feature_word, n_features, flags, d_reads, d_cells): a good one, then every refused form
    forms = [(1, 1, 4, 0, at, at), (0, 2, 1, 1, at, None), (1, 0, 4, 0, at, None), (1, 3, 4, 0, at, None), (1, 1, 0, 0, at, None),
             (1, 1, (1 << 32) + 1, 0, at, None), (1, 1, 4, 2, at, None), (1, 1, 4, 0, at + 4, None), (1, 2, 4, 0, at, at), (1 << 40, 1, 4, 0, at, None)]
    for n, word, nf, flags, d_reads, d_cells in forms:
        totals = (C.c_uint64 * 4)(*[GARBAGE] * 4)
        assert metrics(None, None, n, word, nf, flags, d_reads, None, d_cells, totals, None) != 0
        assert list(totals) == [GARBAGE] * 4, "a refused call leaves the totals alone"
        assert list(words) == [0] * 8
    lims = [fnp.limits(), fnp.limits(min_umis=1), None]          # (min_umis with a NULL d_umis is refused)
    for n, word, nf, _, d_reads, d_cells in forms:
        for lim in lims:
            c = _lib.CFeatureFilterCounts((C.c_uint64 * 3)(*[GARBAGE] * 3), (C.c_uint64 * 4)(*[GARBAGE] * 4), GARBAGE)
            l = _limits_struct(lim) if lim else None
            assert filt(None, None, n, word, nf, d_reads, None, d_cells, C.byref(l) if l else None, None, None, C.byref(c), None) != 0
            assert [*c.features_by_class, *c.reads_by_class, c.reserved] == [GARBAGE] * 8
    if ibu_amd.device_count() > 0:
        return
    table = ibu_amd.FeatureTable(None, None, None, 4, None)
    for call in (lambda: ibu_amd.Context(0).feature_metrics(None, 1, 4), lambda: ibu_amd.Context(0).filter_features(None, 1, table)):
        with pytest.raises(ibu_amd.IbuError) as ei:
            call()
        assert ei.value.kind == "NoDevice"


def test_python_wrapper_refuses_bad_arguments_before_the_library_is_called():
    import ibu_amd
    c = object.__new__(ibu_amd.Context)                           # the context is never looked at
    full = ibu_amd.FeatureTable(1, 1, 1, 4, None)
    for kw in ({"min_reads": -1}, {"max_cells": 1 << 64}, {"min_cells": 3, "max_cells": 2}, {"min_umis": 5, "max_umis": 1}, {"feature_word": 3}):
        with pytest.raises(ValueError):
            ibu_amd.Context.filter_features(c, None, 1, full, **kw)
    with pytest.raises(ValueError):                               # a limit on a column the table does not have
        ibu_amd.Context.filter_features(c, None, 1, ibu_amd.FeatureTable(1, 1, None, 4, None), 2, min_cells=1)
    for args in ((0,), (-1,), ((1 << 32) + 1,), (4, 0), (4, 3)):
        with pytest.raises(ValueError):
            ibu_amd.Context.feature_metrics(c, None, 1, *args)
    with pytest.raises(ValueError):                               # a table of another size, or without cells for feature_word 1
        ibu_amd.Context.feature_metrics(c, None, 1, 5, 1, accumulate_into=full)
    with pytest.raises(ValueError):
        ibu_amd.Context.feature_metrics(c, None, 1, 4, 1, accumulate_into=ibu_amd.FeatureTable(1, 1, None, 4, None))


def test_count_file_example_compiles_with_the_feature_options(tmp_path):
    from ibu_amd import _lib
    src = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    assert "--features=mincells:A[,minumi:B][,maxcells:C]" in src and "--n-features=N" in src and "--feature-table=FILE" in src
    assert "filter_features" in src and "feature_metrics" in src
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    for args in (["--features=mincells:3", "x.ibu"], ["--features=mincells:3", "--n-features=0", "x.ibu"], ["--features=mincells:", "--n-features=9", "x.ibu"],
                 ["--features=minumi:3", "--n-features=9", "x.ibu"], ["--features=mincells:3,bogus:1", "--n-features=9", "x.ibu"],
                 ["--features=mincells:3,mincells:4", "--n-features=9", "x.ibu"], ["--features=mincells:3,", "--n-features=9", "x.ibu"],
                 ["--features=mincells:3x", "--n-features=9", "x.ibu"], ["--features=mincells:99999999999999999999", "--n-features=9", "x.ibu"],
                 ["--features", "--n-features=9", "x.ibu"], ["--n-features=4294967297", "--features=mincells:3", "x.ibu"],
                 ["--n-features=9x", "--features=mincells:3", "x.ibu"], ["--feature-table=t.txt", "x.ibu"], ["--feature-table=", "--n-features=9", "x.ibu"],
                 ["--n-features=9", "x.ibu"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.returncode == 2 and "--features=mincells:A" in r.stderr and "--qc=minfeat:A" in r.stderr, (args, r.stderr)
