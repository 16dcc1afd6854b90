"""The merge of sorted records — what can be checked without a GPU: the numpy statement of the semantics (tests/merge_np.py)
against heapq.merge on tagged tuples, the diagonal search against the statement, the two entry points in every layer of the ABI,
the merge kernels in the code object and their LDS, and the example program's refusals, which come before any device call."""
import ctypes as C
import heapq
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import merge_np as mnp
from tests.count_np import REC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_merge_sorted", "ibu_merge_sorted_runs")


def _sorted_records(rng, n, values):
    """n sorted records whose words are drawn from `values` (few values: long tie runs)."""
    w = values[rng.integers(0, len(values), (n, 3))]
    r = np.ascontiguousarray(w.astype(np.uint64)).view(REC).reshape(-1)
    return np.sort(r, order=["barcode", "umi", "index"])


CASES = [("random", np.array([0, 1, 2, 3, 5, 8, 1 << 31, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], np.uint64)),
         ("ties", np.array([7, 1 << 63], np.uint64)), ("one", np.array([42], np.uint64))]


def _heap_merge(a, b):
    ta = [(*[int(x) for x in r], 0) for r in a.tolist()]
    tb = [(*[int(x) for x in r], 1) for r in b.tolist()]
    return list(heapq.merge(ta, tb))                            # tuples compare word by word, then by tag: a first among equals


@pytest.mark.parametrize("name,values", CASES)
@pytest.mark.parametrize("na,nb", [(0, 0), (0, 5), (5, 0), (1, 1), (17, 40), (64, 64), (100, 3)])
def test_statement_equals_heapq_merge(name, values, na, nb):
    rng = np.random.default_rng(0x3E00 + 131 * na + nb)
    a, b = _sorted_records(rng, na, values), _sorted_records(rng, nb, values)
    out, src = mnp.merge(a, b)
    want = _heap_merge(a, b)
    assert [tuple(int(x) for x in r) for r in out.tolist()] == [t[:3] for t in want]
    assert src.tolist() == [t[3] for t in want]
    assert out.dtype == REC and src.dtype == np.uint8 and len(out) == na + nb
    # stated per record: a[i] lands at i + #{b < a[i]}, b[j] at j + #{a <= b[j]}
    ta, tb = [t[:3] for t in _heap_merge(a, a[:0])], [t[:3] for t in _heap_merge(b, b[:0])]
    pos_a = [i + sum(y < x for y in tb) for i, x in enumerate(ta)]
    pos_b = [j + sum(x <= y for x in ta) for j, y in enumerate(tb)]
    assert sorted(pos_a + pos_b) == list(range(na + nb))
    assert all(src[p] == 0 for p in pos_a) and all(src[p] == 1 for p in pos_b)


@pytest.mark.parametrize("name,values", CASES)
def test_diagonal_counts_the_a_records_of_every_prefix(name, values):
    rng = np.random.default_rng(0x3E10)
    for na, nb in ((0, 7), (7, 0), (13, 29), (40, 40), (33, 2)):
        a, b = _sorted_records(rng, na, values), _sorted_records(rng, nb, values)
        src = mnp.merge(a, b)[1]
        before = np.concatenate([[0], np.cumsum(src == 0)])
        assert [mnp.diagonal(a, b, d) for d in range(na + nb + 1)] == before.tolist(), (name, na, nb)


def test_merge_runs_statement():
    rng = np.random.default_rng(0x3E20)
    for lengths in ([], [5], [0, 0], [3, 0, 9, 1], [10, 20, 30, 5, 0, 7, 1]):
        runs = [_sorted_records(rng, n, CASES[0][1]) for n in lengths]
        recs = np.concatenate(runs) if runs else np.zeros(0, REC)
        got = mnp.merge_runs(recs, lengths)
        assert got.tobytes() == np.sort(recs, order=["barcode", "umi", "index"]).tobytes()


def test_entry_points_exist_in_every_layer():
    from ibu_amd import _lib
    import ibu_amd
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    so = C.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in ibu_hip.h"
        assert hasattr(so, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert re.search(r"pub fn %s\s*\(" % name, ffi), f"{name} is not in ffi.rs"
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    for m in ("merge_sorted", "merge_sorted_runs"):
        assert hasattr(ibu_amd.Context, m), m
        assert re.search(r"pub fn %s\s*\(" % m, lib_rs), m
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "later additions do not bump the revision"
    # a NULL context is an error, never a host computation
    assert so.ibu_merge_sorted(None, None, C.c_size_t(1), None, C.c_size_t(1), None, None, None) != 0
    assert so.ibu_merge_sorted_runs(None, None, None, None, C.c_size_t(2), None) != 0


def test_merge_fails_loudly_without_gpu():
    import ibu_amd
    if ibu_amd.device_count() > 0:
        return                                                   # (the device tests cover the calls)
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Context(0).merge_sorted(None, 0, None, 0)
    assert ei.value.kind == "NoDevice"


def test_merge_kernels_are_in_the_code_object_and_fit_the_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = {k: v for k, v in kernel_resources.all_kernels(_lib.SO_PATH).items() if "ibu_k_merge" in k}
    assert any(k.startswith("ibu_k_merge_partition") for k in ks), sorted(ks)
    tiles = [k for k in ks if "ibu_k_merge<" in k]
    assert len(tiles) == 4, sorted(ks)                           # full stores or bounded ones, with and without source bytes
    for k, v in ks.items():
        assert v.get("group_segment_fixed_size", 0) <= 65536, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
    assert all(ks[k]["group_segment_fixed_size"] > 0 for k in tiles)
    # the tile size the GPU tests mirror
    from tests import test_gpu_merge
    m = re.search(r"kMergeTile\s*=\s*(\d+)\s*;", open(os.path.join(ROOT, "ibu_amd", "csrc", "kernels.h")).read())
    assert m and int(m.group(1)) == test_gpu_merge.T


def _write(path, recs, bc_len=16, umi_len=12, sorted_flag=True):
    import ibu_amd
    h = ibu_amd.Header(bc_len, umi_len)
    if sorted_flag:
        h.set_sorted()
    w = ibu_amd.Writer.from_path(str(path), h)
    w.write_batch(np.ascontiguousarray(recs))
    w.finish()
    w.close()


def test_merge_files_example_compiles_and_refuses_before_any_device_call(tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "merge_files"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "merge_files.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    rng = np.random.default_rng(0x3E30)
    recs = _sorted_records(rng, 100, np.arange(50, dtype=np.uint64))
    _write(tmp_path / "a.ibu", recs)
    _write(tmp_path / "b.ibu", recs)
    _write(tmp_path / "bc8.ibu", recs, bc_len=8)
    _write(tmp_path / "unsorted.ibu", recs[::-1], sorted_flag=False)
    out = tmp_path / "out.ibu"
    run = lambda *args: subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    for args in ((), (out,), (out, tmp_path / "a.ibu"), (out, tmp_path / "a.ibu", tmp_path / "b.ibu", "--no-such-flag")):
        r = run(*args)
        assert r.returncode == 2 and "usage: merge_files" in r.stderr, (args, r.stderr)
    r = run(out, tmp_path / "a.ibu", tmp_path / "bc8.ibu")
    assert r.returncode == 1 and "bc_len" in r.stderr and "NoDevice" not in r.stderr and "device" not in r.stderr.lower(), r.stderr
    r = run(out, tmp_path / "a.ibu", tmp_path / "unsorted.ibu")
    assert r.returncode == 1 and "does not say sorted" in r.stderr and "device" not in r.stderr.lower(), r.stderr
    r = run(out, tmp_path / "a.ibu", tmp_path / "missing.ibu")
    assert r.returncode == 1 and "device" not in r.stderr.lower(), r.stderr
    assert not out.exists(), "a refused call writes no output"
