"""Cell calling (ibu_call_cells) — what can be checked without a GPU: the numpy statement of the semantics (tests/cells_np.py)
against a brute force over the runs and against cases a reader can check by eye, the entry point in every layer of the ABI, the
argument errors that need no device, the loud failure on a box without one, and the example program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cells_np as cnp
from tests import count_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibu_call_cells"


def _same(recs, mode, param, by_reads=False):
    cls, tot = cnp.call_cells(recs, mode, param, by_reads)
    bcls, btot = cnp.brute_force(recs, mode, param, by_reads)
    assert cls.dtype == np.uint8 and cls.tolist() == bcls.tolist(), (mode, param, by_reads)
    assert tot == btot, (mode, param, by_reads, tot, btot)
    n = len(recs)
    assert tot["reads_cells"] + tot["reads_background"] == n == len(cls)
    assert tot["umis_cells"] + tot["umis_background"] == len(count_np.pair_counts(recs)[0]), "the (barcode, umi) runs"
    return cls, tot


def test_numpy_statement_equals_brute_force_where_ties_are_the_rule():
    """A few hundred small inputs, n <= 200, every barcode's metric in 1..4: the cut nearly always falls inside a tie."""
    rng = np.random.default_rng(0x31100)
    cut_in_a_tie = 0
    for case in range(300):
        nb = int(rng.integers(1, 50))
        umis = rng.integers(1, 5, nb)
        by_reads = bool(case & 1)
        recs = cnp.recs_of_metrics(umis, reads_per_umi=1)
        if by_reads:                                              # reads in 1..4 as well: one umi per barcode, repeated
            recs["umi"] = 7
        assert len(recs) <= 200
        if case % 3 == 2:                                         # the runs of unsorted input
            recs = recs[rng.permutation(len(recs))]
        for mode, params in ((cnp.MIN, (0, 1, 2, 4, 5)), (cnp.TOP, (1, 2, nb - 1, nb, nb + 1, 1 << 40)), (cnp.ORDMAG, (1, 99, 100, 101, nb, 100 * nb))):
            for p in params:
                if p == 0 and mode != cnp.MIN:
                    continue
                cls, tot = _same(recs, mode, p, by_reads)
                if mode == cnp.TOP and p < tot["barcodes"]:
                    assert tot["cells"] >= p
                    cut_in_a_tie += tot["cells"] > p
    assert cut_in_a_tie > 200


def _call(umis, mode, param):
    cls, tot = _same(cnp.recs_of_metrics(umis), mode, param)
    return cls.tolist(), tot


def test_hand_written_cases():
    cls, tot = cnp.call_cells(np.zeros(0, cnp.REC), cnp.MIN, 7)
    assert cls.tolist() == [] and tot == dict(dict.fromkeys(cnp.TOTALS, 0), threshold=7)
    assert cnp.call_cells(np.zeros(0, cnp.REC), cnp.TOP, 7)[1] == dict.fromkeys(cnp.TOTALS, 0)
    assert cnp.brute_force(np.zeros(0, cnp.REC), cnp.MIN, 7)[1]["threshold"] == 7
    # T = 0: everything is a cell
    cls, tot = _call([1, 3, 2], cnp.MIN, 0)
    assert cls == [0] * 6 and (tot["cells"], tot["barcodes"], tot["threshold"], tot["baseline"]) == (3, 3, 0, 0)
    cls, tot = _call([1, 3, 2], cnp.MIN, 2)
    assert cls == [1, 0, 0, 0, 0, 0] and (tot["cells"], tot["umis_cells"], tot["umis_background"]) == (2, 5, 1)
    cls, tot = _call([1, 3, 2], cnp.MIN, 4)
    assert cls == [1] * 6 and tot["cells"] == 0 and tot["reads_background"] == 6
    # TOP: ties with the K-th are cells; K > B takes the smallest
    cls, tot = _call([2, 5, 2, 1], cnp.TOP, 2)
    assert tot["threshold"] == 2 and tot["cells"] == 3 and cls == [0] * 9 + [1]
    cls, tot = _call([2, 5, 2, 1], cnp.TOP, 1)
    assert tot["threshold"] == 5 and tot["cells"] == 1
    for k in (4, 5, 1 << 40):
        cls, tot = _call([2, 5, 2, 1], cnp.TOP, k)
        assert tot["threshold"] == 1 and tot["cells"] == 4 and tot["baseline"] == 0
    # ORDMAG: E = 99 picks rank 1, E = 100 rank 2 (E // 100 + 1)
    umis = [1000, 500] + [1] * 198
    cls, tot = _call(umis, cnp.ORDMAG, 99)
    assert (tot["baseline"], tot["threshold"], tot["cells"]) == (1000, 100, 2)
    cls, tot = _call(umis, cnp.ORDMAG, 100)
    assert (tot["baseline"], tot["threshold"], tot["cells"]) == (500, 50, 2)
    cls, tot = _call(umis, cnp.ORDMAG, 199)
    assert (tot["baseline"], tot["threshold"]) == (500, 50)
    cls, tot = _call(umis, cnp.ORDMAG, 200)
    assert (tot["baseline"], tot["threshold"], tot["cells"]) == (1, 1, 200), "rank 3"
    cls, tot = _call(umis, cnp.ORDMAG, 1 << 50)
    assert (tot["baseline"], tot["threshold"]) == (1, 1), "E' = min(E, B)"
    cls, tot = _call([1000, 500], cnp.ORDMAG, 100)
    assert (tot["baseline"], tot["threshold"]) == (1000, 100), "E' = B = 2: rank 1"
    # baseline 10, 11, 19 -> T = 1, 2, 2
    for baseline, T, cells in ((10, 1, 3), (11, 2, 2), (19, 2, 2), (20, 2, 2), (21, 3, 1)):
        cls, tot = _call([baseline, 2, 1], cnp.ORDMAG, 1)
        assert (tot["baseline"], tot["threshold"], tot["cells"]) == (baseline, T, cells)
    # the metric under by_reads; the umis totals stay UMI totals
    recs = cnp.recs_of_metrics([1, 2], reads_per_umi=3)          # reads 3, 6
    cls, tot = _same(recs, cnp.MIN, 3, False)
    assert tot["cells"] == 0
    cls, tot = _same(recs, cnp.MIN, 4, True)
    assert cls.tolist() == [1] * 3 + [0] * 6 and (tot["umis_cells"], tot["umis_background"], tot["reads_cells"]) == (2, 1, 6)
    # an interrupted barcode on unsorted input is two barcodes
    recs = np.array([(5, 1, 0), (5, 2, 0), (6, 1, 0), (5, 3, 0)], cnp.REC)
    cls, tot = _same(recs, cnp.MIN, 2)
    assert cls.tolist() == [0, 0, 1, 1] and tot["barcodes"] == 3
    # a umi that returns inside a barcode counts again
    recs = np.array([(5, 1, 0), (5, 2, 0), (5, 1, 0)], cnp.REC)
    assert _same(recs, cnp.MIN, 3)[1]["cells"] == 1


def test_the_knee_fixture_has_a_knee():
    recs = cnp.knee(np.random.default_rng(0x31200), 100, 3000)
    assert recs.tobytes() == count_np.sort_records(recs).tobytes()
    cls, tot = cnp.call_cells(recs, cnp.ORDMAG, 100)
    assert tot["barcodes"] == 3100 and tot["cells"] == 100 and 20 <= tot["threshold"] <= 40


def test_entry_point_exists_in_every_layer():
    from ibu_amd import _lib
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    so = C.CDLL(_lib.SO_PATH)
    assert re.search(r"\b%s\s*\(" % NAME, code), "not declared in ibu_hip.h"
    assert hasattr(so, NAME), "not exported"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 9
    assert re.search(r"pub fn %s\s*\(" % NAME, ffi)
    # the selection's test hook is exported and nothing more: no declaration, no binding
    assert hasattr(so, "ibu_test_rank_select") and "rank_select" not in header and "rank_select" not in ffi and "ibu_test_rank_select" not in _lib.SIGNATURES
    assert "pub struct ibu_cell_counts_t" in ffi
    assert C.sizeof(_lib.CCellCounts) == 64 and tuple(f for f, _ in _lib.CCellCounts._fields_) == cnp.TOTALS
    for name, value in (("IBU_CELL", "0"), ("IBU_CELL_BACKGROUND", "1"), ("IBU_CELLS_MIN", "0u"), ("IBU_CELLS_TOP", "1u"), ("IBU_CELLS_ORDMAG", "2u"),
                        ("IBU_CELLS_BY_READS", "1u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    import ibu_amd
    assert (ibu_amd.CELL, ibu_amd.CELL_BACKGROUND, ibu_amd.CELLS_MIN, ibu_amd.CELLS_TOP, ibu_amd.CELLS_ORDMAG, ibu_amd.CELLS_BY_READS) == (0, 1, 0, 1, 2, 1)
    assert (cnp.CELL, cnp.BACKGROUND, cnp.MIN, cnp.TOP, cnp.ORDMAG, cnp.BY_READS) == (0, 1, 0, 1, 2, 1)
    assert ibu_amd.CellCounts._fields == cnp.TOTALS
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    assert re.search(r"pub fn call_cells\s*\(", lib_rs) and re.search(r"\bcall_cells\s*\(", hpp)
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "a new entry point changes no signature"
    # the struct has the size and the field order the header compiles to
    fields = re.search(r"typedef struct ibu_cell_counts \{(.*?)\}", code, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == cnp.TOTALS


def test_kernels_are_in_the_code_object_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = kernel_resources.all_kernels(_lib.SO_PATH)
    for k in ("ibu_k_cells_emit", "ibu_k_cells_table", "ibu_k_select_hist", "ibu_k_select_narrow", "ibu_k_cells_verdict",
              "ibu::ibu_k_class_fill<true>", "ibu::ibu_k_class_fill<false>"):
        assert k in ks, k
        assert ks[k].get("private_segment_fixed_size", 0) == 0 and not ks[k].get("uses_dynamic_stack", 0), (k, ks[k])


def test_python_wrapper_wants_exactly_one_mode():
    """Refused before the library is called: the context is never looked at."""
    import ibu_amd
    c = object.__new__(ibu_amd.Context)
    for kw in ({}, {"min_umis": 1, "top": 2}, {"top": 1, "expected_cells": 3}, {"min_umis": 0, "top": 1, "expected_cells": 1}):
        with pytest.raises(ValueError, match="exactly one of"):
            ibu_amd.Context.call_cells(c, None, 1, **kw)
    with pytest.raises(ValueError):
        ibu_amd.Context.call_cells(c, None, 1, min_umis=-1)


def test_call_cells_fails_loudly_without_gpu():
    """A NULL context is an error whatever the other arguments say, never a host computation; without a device the Python
    Context cannot exist."""
    import ibu_amd
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    fn = so.ibu_call_cells
    fn.restype, fn.argtypes = _lib.SIGNATURES[NAME]
    garbage = 0x5A5A5A5A5A5A5A5A
    c = _lib.CCellCounts(*[garbage] * 8)
    for n, mode, param, flags in ((1, 0, 1, 0), (0, 0, 0, 0), (1, 3, 1, 0), (1, 1, 0, 0), (1, 2, 0, 0), (1, 0, 1, 2), (1 << 40, 0, 1, 0)):
        assert fn(None, None, n, mode, param, flags, None, C.byref(c), None) != 0
        assert all(getattr(c, f) == garbage for f in cnp.TOTALS), "a refused call leaves the totals alone"
    sel = so.ibu_test_rank_select
    sel.restype, sel.argtypes = C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    v = C.c_uint64(garbage)
    assert sel(None, None, 1, 1, C.byref(v), None) != 0 and v.value == garbage
    if ibu_amd.device_count() > 0:
        return
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Context(0).call_cells(None, 1, min_umis=1)
    assert ei.value.kind == "NoDevice"


def test_count_file_example_compiles_with_the_cells_option(tmp_path):
    from ibu_amd import _lib
    src = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    assert "--cells=min:T|top:K|expected:E" in src and "call_cells" in src
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    for args in ([], ["--cells=top:3"], ["--cells=bogus:3", "x.ibu"], ["--cells=top:0", "x.ibu"], ["--cells=min:", "x.ibu"], ["--cells", "x.ibu"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.returncode == 2 and "usage: count_file" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("n,rpm", [(2_003, 4), (10_007, 4), (123_457, 4), (123_456, 3), (250_001, 5)])
def test_the_benchmark_lays_exactly_n_records(n, rpm):
    """tools/aggbench.py --cells checks the library against the layout it laid: replayed here on the CPU, the layout's rows add up to
    n and the numpy statement finds in its records exactly the barcodes, molecules and cells the layout says."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import aggbench
    umis, starts, ends, n_cells, n_bg = aggbench.knee_layout(torch, n, rpm, "cpu")
    assert int(ends[-1]) == n and int(starts[0]) == 0 and len(umis) == n_cells + n_bg and bool((ends > starts).all())
    bc, um = aggbench.knee_fill(torch, torch.arange(n, dtype=torch.int64), starts, ends, rpm)
    recs = np.zeros(n, cnp.REC)
    recs["barcode"], recs["umi"] = bc.numpy().astype(np.uint64), um.numpy().astype(np.uint64)
    assert recs.tobytes() == count_np.sort_records(recs).tobytes()
    first, reads, got_umis = cnp.barcode_table(recs)
    assert first.tolist() == starts.tolist() and reads.tolist() == (ends - starts).tolist() and got_umis.tolist() == umis.tolist()
    tot = cnp.call_cells(recs, cnp.ORDMAG, n_cells)[1]
    assert tot["barcodes"] == n_cells + n_bg and tot["cells"] == int((umis >= tot["threshold"]).sum()) == n_cells
    assert tot["umis_cells"] + tot["umis_background"] == int(umis.sum())
