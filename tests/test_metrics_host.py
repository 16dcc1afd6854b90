"""Per-barcode QC metrics and the barcode filter (ibu_barcode_metrics, ibu_filter_barcodes) — what can be checked without a GPU:
the numpy statement of the semantics (tests/metrics_np.py) against a brute force over the barcodes and against cases a reader can
check by eye, the entry points in every layer of the ABI, the kernels' resources, the argument errors that need no device, the loud
failure on a box without one, and the example program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import metrics_np as mnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_barcode_metrics", "ibu_filter_barcodes")
GARBAGE = 0x5A5A5A5A5A5A5A5A
# values on either side of the set sizes the tests use (1, 64, 65 bits), of the word boundary (63 / 64), and one above 2^32
PALETTE = np.array([0, 1, 62, 63, 64, 65, 66, (1 << 32) + 7], np.uint64)


def _random_records(rng, n):
    r = np.zeros(n, mnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    w[:, 0] = np.sort(rng.integers(0, max(n // 4, 1) + 1, n)).astype(np.uint64)
    w[:, 1] = PALETTE[rng.integers(0, len(PALETTE), n) // 2 * 2 % len(PALETTE)]
    w[:, 2] = PALETTE[rng.integers(0, len(PALETTE), n)]
    if rng.integers(0, 3):                                       # mostly sorted inside the barcodes, sometimes the runs as they stand
        order = np.lexsort((w[:, 2], w[:, 1], w[:, 0]))
        r = r[order]
    return r


def _random_set(rng):
    bits = int(rng.choice([0, 1, 63, 64, 65, 66, 128, 200]))
    if bits == 0:
        return None, 0
    values = [v for v in range(bits) if rng.integers(0, 2)]
    if rng.integers(0, 2):
        values = sorted(set(values) | {bits - 1})                 # the top bit
    return mnp.bitmap(values, bits), bits


def test_numpy_statement_equals_brute_force():
    rng = np.random.default_rng(0x41100)
    classes_seen = set()
    for case in range(300):
        n = int(rng.integers(0, 120))
        recs = _random_records(rng, n)
        words, bits = _random_set(rng)
        set_word = 1 + (case & 1)
        table = mnp.barcode_metrics(recs, words, bits, set_word)
        want = mnp.brute_force(recs, words, bits, set_word)
        assert [tuple(int(c[k]) for c in table) for k in range(len(table[0]))] == want, case
        assert all(c.dtype == np.uint64 for c in table)
        assert int(table[1].sum()) == n and bool((table[2] <= table[3]).all()) and bool((table[5] <= table[4]).all())
        lim = mnp.limits(min_reads=int(rng.integers(0, 3)), max_reads=int(rng.integers(0, 8)), min_pairs=int(rng.integers(0, 3)),
                         max_pairs=int(rng.integers(0, 4)), min_triples=int(rng.integers(0, 3)), max_triples=int(rng.integers(0, 6)),
                         set_num=int(rng.integers(0, 3)), set_den=int(rng.integers(0, 4)) + 2, set_of=int(rng.integers(0, 2)))
        if case % 5 == 0:
            lim["set_den"] = lim["set_num"] = 0
        cls, tot = mnp.filter_barcodes(recs, words, bits, set_word, lim)
        _, bcls, btot = mnp.brute_force(recs, words, bits, set_word, lim)
        assert cls.dtype == np.uint8 and cls.tolist() == bcls.tolist() and tot == btot, (case, tot, btot)
        assert sum(tot["reads_by_class"]) == n and sum(tot["barcodes_by_class"]) == tot["barcodes"]
        classes_seen |= set(cls.tolist())
    assert classes_seen == {0, 1, 2, 3}


def _recs(rows):
    return np.array(rows, mnp.REC)


def test_hand_written_cases():
    # barcode 7: reads 5, pairs (7,1) (7,2) (7,64): 3, triples 4; barcode 9: one record
    recs = _recs([(7, 1, 10), (7, 1, 10), (7, 1, 63), (7, 2, 63), (7, 64, 5), (9, 1, 63)])
    assert [c.tolist() for c in mnp.barcode_metrics(recs)] == [[7, 9], [5, 1], [3, 1], [4, 1], [0, 0], [0, 0]]
    w64 = mnp.bitmap([1, 63], 64)                                 # 64 bits: the value 64 = set_bits is not in the set
    assert [c.tolist() for c in mnp.barcode_metrics(recs, w64, 64, 1)][4:] == [[3, 1], [2, 1]]
    assert [c.tolist() for c in mnp.barcode_metrics(recs, w64, 64, 2)][4:] == [[2, 1], [2, 1]]
    w65 = mnp.bitmap([64], 65)                                    # bit 0 of the second word
    assert [c.tolist() for c in mnp.barcode_metrics(recs, w65, 65, 1)][4:] == [[1, 0], [1, 0]]
    assert [c.tolist() for c in mnp.barcode_metrics(recs, mnp.bitmap([0], 1), 1, 1)][4:] == [[0, 0], [0, 0]]
    big = _recs([(1, (1 << 32) + 7, 0), (1, 7, 0)])               # a value of 2^32 and more is in no set: the low bits do not alias
    assert mnp.barcode_metrics(big, mnp.bitmap([7], 8), 8, 1)[4].tolist() == [1]
    # an interrupted barcode is two barcodes; a pair that returns counts again
    recs2 = _recs([(5, 1, 0), (6, 1, 0), (5, 1, 0), (5, 2, 0), (5, 1, 0)])
    assert [c.tolist() for c in mnp.barcode_metrics(recs2)][:4] == [[5, 6, 5], [1, 1, 3], [1, 1, 3], [1, 1, 3]]
    assert all(len(c) == 0 for c in mnp.barcode_metrics(np.zeros(0, mnp.REC)))

    def classes(lim, words=w64, bits=64, set_word=1):
        cls, tot = mnp.filter_barcodes(recs, words, bits, set_word, lim)
        return [int(cls[0]), int(cls[5])], tot
    # a zeroed struct passes everything; a maximum of 0 is no maximum
    got, tot = classes(mnp.limits())
    assert got == [0, 0] and tot == {"barcodes": 2, "barcodes_by_class": (2, 0, 0, 0), "reads_by_class": (6, 0, 0, 0), "triples_passed": 5,
                                     "set_triples_passed": 3, "reserved": 0}
    assert classes(mnp.limits(max_reads=0, max_pairs=0, max_triples=0, min_reads=1))[0] == [0, 0]
    # each limit alone
    assert classes(mnp.limits(min_reads=2))[0] == [0, 1] and classes(mnp.limits(min_pairs=2))[0] == [0, 1]
    assert classes(mnp.limits(min_triples=5))[0] == [1, 1]
    assert classes(mnp.limits(max_reads=4))[0] == [2, 0] and classes(mnp.limits(max_pairs=2))[0] == [2, 0]
    assert classes(mnp.limits(max_triples=4))[0] == [0, 0] and classes(mnp.limits(max_triples=3))[0] == [2, 0]
    # the share: barcode 7 has 3 of 5 reads and 2 of 4 triples in the set, barcode 9 all of its one
    assert classes(mnp.limits(set_num=3, set_den=5))[0] == [0, 3], "equality passes"
    assert classes(mnp.limits(set_num=59, set_den=100))[0] == [3, 3]
    assert classes(mnp.limits(set_num=1, set_den=2, set_of=1))[0] == [0, 3], "equality passes, of triples"
    assert classes(mnp.limits(set_num=1, set_den=2, set_of=0))[0] == [3, 3]
    assert classes(mnp.limits(set_num=1, set_den=1))[0] == [0, 0] and classes(mnp.limits(set_num=0, set_den=1))[0] == [3, 3]
    assert classes(mnp.limits(set_num=0, set_den=0))[0] == [0, 0], "set_den == 0: no set test"
    assert classes(mnp.limits(set_num=0, set_den=1), None, 0)[0] == [0, 0], "the empty set"
    # the first class that applies wins: LOW before HIGH before SET
    got, tot = classes(mnp.limits(min_triples=5, max_reads=4, set_num=0, set_den=1))
    assert got == [1, 1]
    got, tot = classes(mnp.limits(min_reads=2, max_reads=4, set_num=0, set_den=1))
    assert got == [2, 1] and tot["barcodes_by_class"] == (0, 1, 1, 0) and tot["reads_by_class"] == (0, 1, 5, 0) and tot["triples_passed"] == 0
    got, tot = classes(mnp.limits(max_reads=4, set_num=0, set_den=1))
    assert got == [2, 3]
    got, tot = classes(mnp.limits(set_num=3, set_den=5))
    assert tot["triples_passed"] == 4 and tot["set_triples_passed"] == 2 and tot["reads_by_class"] == (5, 0, 0, 1)


def test_bitmap_helper_of_the_package():
    import ibu_amd
    for values, bits in (([], 0), ([0], 1), ([63], 64), ([0, 63, 64], 65), ([5, 5, 100], 200)):
        assert ibu_amd.feature_bitmap_words(values, bits).tobytes() == mnp.bitmap(values, bits).tobytes()
    assert ibu_amd.feature_bitmap_words([], 0).dtype == np.uint64
    with pytest.raises(ValueError):
        ibu_amd.feature_bitmap_words([64], 64)
    with pytest.raises(ValueError):
        ibu_amd.feature_bitmap_words([], (1 << 32) + 1)


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
    for name, nargs in zip(NAMES, (15, 10)):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in ibu_hip.h"
        assert hasattr(so, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"pub fn %s\s*\(" % name, ffi)
        short = name[4:]
        assert re.search(r"pub fn %s\s*\(" % short, lib_rs) and re.search(r"\b%s\s*\(" % short, hpp) and hasattr(ibu_amd.Context, short)
    assert hasattr(ibu_amd.Context, "feature_bitmap")
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "new entry points change no signature"
    for k, name in enumerate(("IBU_BARCODE_PASS", "IBU_BARCODE_LOW", "IBU_BARCODE_HIGH", "IBU_BARCODE_SET")):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, k), code), name
    assert (ibu_amd.BARCODE_PASS, ibu_amd.BARCODE_LOW, ibu_amd.BARCODE_HIGH, ibu_amd.BARCODE_SET) == (0, 1, 2, 3) == (mnp.PASS, mnp.LOW, mnp.HIGH, mnp.SET)
    assert ibu_amd.BarcodeMetrics._fields == mnp.COLUMNS and ibu_amd.BarcodeFilterCounts._fields == mnp.TOTALS[:-1]
    # the structs: the field order of the header in ctypes and Rust, and the sizes and offsets the header compiles to
    for cname, twin, fields in (("ibu_barcode_limits", _lib.CBarcodeLimits, mnp.LIMITS), ("ibu_barcode_filter_counts", _lib.CBarcodeFilterCounts, mnp.TOTALS)):
        assert _struct_fields(code, cname) == fields == tuple(f for f, _ in twin._fields_), cname
        rust = re.search(r"pub struct %s_t \{(.*?)\}" % cname, ffi, flags=re.S).group(1)
        assert tuple(re.findall(r"pub ([a-z_]+):", rust)) == fields, cname
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ibu_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ibu_barcode_limits_t), offsetof(ibu_barcode_limits_t, set_of),\n'
                   "         sizeof(ibu_barcode_filter_counts_t), offsetof(ibu_barcode_filter_counts_t, reads_by_class),\n"
                   "         offsetof(ibu_barcode_filter_counts_t, triples_passed), offsetof(ibu_barcode_filter_counts_t, reserved));\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    L, F = _lib.CBarcodeLimits, _lib.CBarcodeFilterCounts
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == \
        [C.sizeof(L), L.set_of.offset, C.sizeof(F), F.reads_by_class.offset, F.triples_passed.offset, F.reserved.offset] == [72, 64, 96, 40, 72, 88]


def _kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    return kernel_resources.all_kernels(_lib.SO_PATH)


def test_kernels_are_in_the_code_object_without_scratch():
    ks = _kernels()
    for k in ("ibu_k_metrics_count", "ibu_k_metrics_emit", "ibu_k_metrics_table", "ibu_k_metrics_verdict"):
        assert k in ks, k
        assert ks[k].get("private_segment_fixed_size", 0) == 0 and not ks[k].get("uses_dynamic_stack", 0), (k, ks[k])


# (VGPRs, SGPRs, LDS bytes) of the kernels that run the walk of runs_walk.hpp, as the commit before the walk got its `words` hook
# compiled them: the hook has an empty body in every sink but the metrics', so nothing may move
WALK_KERNELS = {
    "ibu_k_cells_emit": (48, 53, 12288),
    "ibu::ibu_k_class_fill<true>": (34, 32, 0),
    "ibu::ibu_k_class_fill<false>": (36, 32, 0),
    "ibu_k_pairs_count": (44, 46, 12288),
    "ibu_k_pairs_emit": (54, 62, 12288),
    "ibu_k_saturation_walk": (80, 98, 14336),
    "ibu_k_runs_scan": (26, 47, 16),                          # (the scan both the aggregations and the metrics launch)
}


def test_the_walk_kernels_kept_their_registers_and_lds():
    ks = _kernels()
    got = {k: (ks[k]["vgpr_count"], ks[k]["sgpr_count"], ks[k].get("group_segment_fixed_size", 0)) for k in WALK_KERNELS}
    assert got == WALK_KERNELS


def test_refused_calls_touch_nothing_and_no_device_is_loud():
    """A NULL context is an error whatever the other arguments say, and so is every refused combination: non-zero, with
    *n_barcodes and `counts` as they were.  Without a device the Python Context cannot exist."""
    import ibu_amd
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    metrics, filt = so.ibu_barcode_metrics, so.ibu_filter_barcodes
    metrics.restype, metrics.argtypes = _lib.SIGNATURES[NAMES[0]]
    filt.restype, filt.argtypes = _lib.SIGNATURES[NAMES[1]]
    words = (C.c_uint64 * 4)()
    at = C.addressof(words)
    # (n, d_set, set_bits, set_word): a good one, then every refused set
    sets = [(1, None, 0, 1), (0, None, 0, 2), (1, None, 0, 0), (1, None, 0, 3), (1, at, (1 << 32) + 1, 1), (1, None, 1, 1), (1, at + 4, 64, 1),
            (1 << 40, None, 0, 1)]
    for n, d_set, bits, word in sets:
        nb = C.c_size_t(GARBAGE)
        assert metrics(None, None, n, d_set, bits, word, None, None, None, None, None, None, 0, C.byref(nb), None) != 0
        assert nb.value == GARBAGE, "a refused call leaves *n_barcodes alone"
        assert metrics(None, None, n, d_set, bits, word, None, None, None, None, None, None, 0, None, None) != 0
    lims = [mnp.limits(), mnp.limits(set_of=2), mnp.limits(set_num=2, set_den=1), mnp.limits(set_num=1, set_den=1 << 24), None]
    for n, d_set, bits, word in sets:
        for lim in lims:
            c = _lib.CBarcodeFilterCounts(GARBAGE, (C.c_uint64 * 4)(*[GARBAGE] * 4), (C.c_uint64 * 4)(*[GARBAGE] * 4), GARBAGE, GARBAGE, GARBAGE)
            l = _lib.CBarcodeLimits(*[lim[f] for f in mnp.LIMITS]) if lim else None
            assert filt(None, None, n, d_set, bits, word, C.byref(l) if l else None, None, C.byref(c), None) != 0
            assert [c.barcodes, *c.barcodes_by_class, *c.reads_by_class, c.triples_passed, c.set_triples_passed, c.reserved] == [GARBAGE] * 12
    if ibu_amd.device_count() > 0:
        return
    for call in (lambda: ibu_amd.Context(0).barcode_metrics(None, 1), lambda: ibu_amd.Context(0).filter_barcodes(None, 1, min_pairs=1),
                 lambda: ibu_amd.Context(0).feature_bitmap([1], 8)):
        with pytest.raises(ibu_amd.IbuError) as ei:
            call()
        assert ei.value.kind == "NoDevice"


def test_python_wrapper_refuses_bad_limits_before_the_library_is_called():
    import ibu_amd
    c = object.__new__(ibu_amd.Context)                           # the context is never looked at
    for kw in ({"set_of": "umis"}, {"max_set_fraction": (2, 1)}, {"max_set_fraction": (1, 0)}, {"max_set_fraction": (1, 1 << 24)}, {"min_reads": -1},
               {"max_pairs": 1 << 64}):
        with pytest.raises(ValueError):
            ibu_amd.Context.filter_barcodes(c, None, 1, **kw)


def test_count_file_example_compiles_with_the_qc_options(tmp_path):
    from ibu_amd import _lib
    src = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    assert "--qc=minfeat:A[,maxfeat:B][,minumi:C][,maxset:NUM/DEN]" in src and "--set=FILE" in src and "filter_barcodes" in src
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    old_usage = ("usage: count_file [--resolve | --resolve=first] [--cells=min:T|top:K|expected:E] [--subsample=F[:seed]] [--saturation=K] "
                 "IN [WHITELIST.txt]")
    for args in ([], ["--qc=minfeat:3"], ["--qc=maxfeat:3", "x.ibu"], ["--qc=minfeat:", "x.ibu"], ["--qc=minfeat:3,", "x.ibu"], ["--qc", "x.ibu"],
                 ["--qc=minfeat:3,minfeat:4", "x.ibu"], ["--qc=minfeat:3,maxset:2/1", "x.ibu"], ["--qc=minfeat:3,maxset:1/0", "x.ibu"],
                 ["--qc=minfeat:3,maxset:1", "x.ibu"], ["--qc=minfeat:3,maxset:1/16777216", "x.ibu"], ["--qc=minfeat:3,bogus:1", "x.ibu"],
                 ["--qc=minfeat:3x", "x.ibu"], ["--qc=minfeat:99999999999999999999", "x.ibu"], ["--qc=minfeat:1,maxset:1/99999999999999999999", "x.ibu"], ["--set=genes.txt", "x.ibu"], ["--set=", "--qc=minfeat:3", "x.ibu"], ["--set", "--qc=minfeat:3", "x.ibu"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.returncode == 2 and old_usage in r.stderr and "--qc=minfeat:A" in r.stderr, (args, r.stderr)
