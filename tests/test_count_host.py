"""The count matrix — what can be checked without a GPU: the numpy statement of the semantics (tests/count_np.py) against a
brute-force dict of sets and against cases a reader can check by eye, the three entry points in every layer of the ABI, the
loud failure on a box without a device, and the example program against include/ibu.hpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import count_np as cnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_records_swap_umi_index", "ibu_pair_counts", "ibu_count_matrix")


def recs_of(rows):
    r = np.zeros(len(rows), cnp.REC)
    for k, (b, u, i) in enumerate(rows):
        r[k] = (b, u, i)
    return r


@pytest.mark.parametrize("bc_len,n", [(4, 3000), (16, 3000), (32, 2000)])
def test_numpy_statement_equals_brute_force(bc_len, n):
    rng = np.random.default_rng(0xC0077 + bc_len)
    recs = cnp.make_records(rng, n, bc_len, n_barcodes=30, n_indices=10, n_umis=8)
    (b, i, reads, umis), s = cnp.count_matrix(recs)
    bb, bi, breads, bumis = cnp.brute_force_matrix(recs)
    assert (b == bb).all() and (i == bi).all() and (reads == breads).all() and (umis == bumis).all()
    assert int(reads.sum()) == n
    # the fixture is what it claims to be
    print("entries", len(b), "molecules", int(umis.sum()), "reads per molecule", n / int(umis.sum()))
    assert n / int(umis.sum()) > 1.5, "mean reads per molecule"
    assert (umis == 1).any() and (umis > 1).any(), "pairs with one molecule and with several"
    mb, mu, mreads, midx = cnp.pair_counts(cnp.sort_records(recs))       # the molecule view: (barcode, umi) with distinct indices
    assert (midx >= 2).any(), "a (barcode, umi) seen with two indices"
    assert int(mreads.sum()) == n and int(midx.sum()) == int(umis.sum())  # the same triples counted from either side
    assert (recs["umi"] >> np.uint64(63)).any() and (recs["index"] >> np.uint64(63)).any(), "words with bit 63 set"
    if bc_len == 32:
        assert (recs["barcode"] >> np.uint64(63)).any()
    # swap is its own inverse and moves nothing else
    assert cnp.swap(cnp.swap(recs)).tobytes() == recs.tobytes()
    sw = cnp.swap(recs)
    assert (sw["barcode"] == recs["barcode"]).all() and (sw["umi"] == recs["index"]).all() and (sw["index"] == recs["umi"]).all()
    # the order of the input does not enter the matrix
    (b2, i2, r2, u2), _ = cnp.count_matrix(recs[::-1])
    assert (b2 == b).all() and (i2 == i).all() and (r2 == reads).all() and (u2 == umis).all()
    assert (np.diff(s.view(np.uint64).reshape(-1, 3)[:, 0].astype(object)) >= 0).all()


def test_hand_written_cases():
    e = cnp.pair_counts(np.zeros(0, cnp.REC))
    assert all(len(x) == 0 for x in e)
    one = cnp.pair_counts(recs_of([(7, 8, 9)]))
    assert [x.tolist() for x in one] == [[7], [8], [1], [1]]
    same = cnp.pair_counts(recs_of([(1, 2, 3)] * 5))
    assert [x.tolist() for x in same] == [[1], [2], [5], [1]]
    distinct = cnp.pair_counts(recs_of([(1, 1, 0), (1, 2, 0), (2, 2, 0), (3, 0, 0)]))
    assert [x.tolist() for x in distinct] == [[1, 1, 2, 3], [1, 2, 2, 0], [1, 1, 1, 1], [1, 1, 1, 1]]
    # one pair whose third word goes 5 5 6 5: three positions differ from the record before them (the first counts) — on
    # unsorted input this is the run-length figure, not the number of distinct values (which is two)
    split = cnp.pair_counts(recs_of([(1, 1, 5), (1, 1, 5), (1, 1, 6), (1, 1, 5), (1, 2, 5)]))
    assert [x.tolist() for x in split] == [[1, 1], [1, 2], [4, 1], [3, 1]]
    # a pair that is interrupted and returns is two entries
    back = cnp.pair_counts(recs_of([(1, 1, 0), (2, 1, 0), (1, 1, 0)]))
    assert [x.tolist() for x in back] == [[1, 2, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    # the count matrix of six reads: barcode 10 has index 0 (UMIs 7, 7, 8: three reads, two molecules) and index 1 (one read);
    # barcode 20 has index 0 twice with one UMI.  Bit 63 orders as unsigned.
    hi = 1 << 63
    recs = recs_of([(20, 5, 0), (10, 7, 0), (10, 3, 1), (10, 8, 0), (20, 5, 0), (10, 7, 0), (hi, 1, hi)])
    (b, i, reads, umis), s = cnp.count_matrix(recs)
    assert b.tolist() == [10, 10, 20, hi] and i.tolist() == [0, 1, 0, hi]
    assert reads.tolist() == [3, 1, 2, 1] and umis.tolist() == [2, 1, 1, 1]
    assert s.tolist() == [(10, 0, 7), (10, 0, 7), (10, 0, 8), (10, 1, 3), (20, 0, 5), (20, 0, 5), (hi, hi, 1)]
    assert cnp.swap(recs_of([(1, 2, 3)])).tolist() == [(1, 3, 2)]


def test_entry_points_exist_in_every_layer():
    from ibu_amd import _lib
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    so = C.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in ibu_hip.h"
        assert hasattr(so, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert re.search(r"pub fn %s\s*\(" % name, ffi), f"{name} is not in ffi.rs"
    assert re.search(r"#define\s+IBU_COUNT_LEAVE_SWAPPED\s+1u?\b", code)
    import ibu_amd
    assert ibu_amd.COUNT_LEAVE_SWAPPED == 1
    for m in ("swap_umi_index", "pair_counts", "count_matrix"):
        assert hasattr(ibu_amd.Context, m), m
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    for m in ("swap_umi_index", "pair_counts", "count_matrix"):
        assert re.search(r"pub fn %s\s*\(" % m, lib_rs), m
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6


def test_kernels_are_in_the_code_object():
    from ibu_amd import _lib
    out = subprocess.run(["strings", "-a", _lib.SO_PATH], capture_output=True, text=True).stdout
    for k in ("ibu_k_swap_fields", "ibu_k_pairs_count", "ibu_k_pairs_emit"):
        assert k in out, k


def test_count_matrix_fails_loudly_without_gpu():
    """No device: NoDevice from the library — there is no host form of the count matrix to fall back to."""
    import ibu_amd
    if ibu_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Context(0).count_matrix(None, None, 1)
    assert ei.value.kind == "NoDevice"
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    n = C.c_size_t()
    for call in (lambda: so.ibu_records_swap_umi_index(None, None, None, C.c_size_t(1), None),
                 lambda: so.ibu_pair_counts(None, None, C.c_size_t(1), None, None, None, None, C.c_size_t(0), C.byref(n), None, None),
                 lambda: so.ibu_count_matrix(None, None, None, C.c_size_t(1), 0, None, None, None, None, C.c_size_t(0), C.byref(n), None, None)):
        assert call() != 0, "a NULL context is an error, never a host computation"


def test_count_file_example_compiles(tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: count_file" in r.stderr
