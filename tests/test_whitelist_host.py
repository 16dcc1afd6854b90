"""Barcode correction against a whitelist — what can be checked without a GPU: the numpy statement of the semantics
(tests/whitelist_np.py) against a brute-force set / Hamming loop, the five entry points in every layer of the ABI, the loud
failure on a box without a device, and the example program against include/ibu.hpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import whitelist_np as wnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_whitelist_create", "ibu_whitelist_info", "ibu_whitelist_destroy", "ibu_correct_barcodes", "ibu_select_records")


@pytest.mark.parametrize("bc_len,w,n", [(4, 40, 3000), (16, 300, 3000), (32, 300, 2000)])
def test_numpy_statement_equals_brute_force(bc_len, w, n):
    # (40 of the 256 four-base codes leave about a tenth of the space without an entry at distance <= 1, so the unmatched share of
    # that case hovers around 2-3 % from draw to draw; the share assertion below guards the FIXTURE, and this seed is one whose draw
    # has every class)
    rng = np.random.default_rng(0x1B00200 + bc_len)
    wl, bc = wnp.make_case(rng, bc_len, w, n)
    assert len(wl) >= w - 2
    a, b = int(wl[0]), int(wl[1])
    d = a ^ b
    assert bin((d | (d >> 1)) & 0x5555555555555555).count("1") == 2, "the planted pair is at distance 2"
    if bc_len < 32:
        assert (bc >> np.uint64(2 * bc_len)).any(), "junk bits above 2*bc_len are part of the input"
    for mm in (1, 0):
        cls, out = wnp.classify(bc, wl, bc_len, mm)
        cls_b, out_b = wnp.brute_force(bc, wl, bc_len, mm)
        assert (cls == cls_b).all() and (out == out_b).all()
    cls, out = wnp.classify(bc, wl, bc_len, 1)
    share = np.bincount(cls, minlength=4) / n
    print("class counts", np.bincount(cls, minlength=4))
    assert (share >= 0.02).all(), share          # every class is really exercised
    m = wnp.mask(bc_len)
    assert ((out & ~m) == (bc & ~m)).all()       # the bits above 2*bc_len are carried along
    assert (out[cls != 1] == bc[cls != 1]).all() and (out[cls == 1] != bc[cls == 1]).all()
    # the whitelist's order and duplicates do not enter
    cls2, out2 = wnp.classify(bc, np.concatenate([wl[::-1], wl[:7]]), bc_len, 1)
    assert (cls2 == cls).all() and (out2 == out).all()
    assert set(np.unique(wnp.classify(bc, wl, bc_len, 0)[0])) <= {0, 3}


def test_one_base_barcodes_class_by_class():
    """bc_len = 1: every barcode is a neighbour of every other one, so class 3 cannot occur."""
    bc = np.arange(4, dtype=np.uint64)
    cls, out = wnp.classify(bc, [0, 3], 1)
    assert cls.tolist() == [0, 2, 2, 0] and (out == bc).all()          # 1 and 2 have both entries at distance 1
    cls, out = wnp.classify(bc, [2], 1)
    assert cls.tolist() == [1, 1, 0, 1] and out.tolist() == [2, 2, 2, 2]
    cls, out = wnp.classify(bc | np.uint64(0xF0), [2], 1)              # junk above bit 2 stays
    assert cls.tolist() == [1, 1, 0, 1] and out.tolist() == [0xF2] * 4
    for wl in ([0], [1, 2], [0, 1, 2, 3], [3, 3]):
        assert 3 not in wnp.classify(bc, wl, 1)[0]
        assert (wnp.classify(bc, wl, 1)[0] == wnp.brute_force(bc, wl, 1)[0]).all()


def test_select_statement():
    recs = np.zeros(6, wnp.REC)
    recs["index"] = np.arange(6)
    cls = np.array([0, 1, 2, 3, 9, 0], np.uint8)
    assert wnp.select(recs, cls, 0b0011)["index"].tolist() == [0, 1, 5]
    assert wnp.select(recs, cls, 0b1100)["index"].tolist() == [2, 3]
    assert wnp.select(recs, cls, 0xFFFF)["index"].tolist() == [0, 1, 2, 3, 5]   # classes above 7 are never kept


def test_entry_points_exist_in_every_layer(tmp_path):
    """Header, shared library, ctypes table, Rust extern block; ibu_correct_counts_t is 32 bytes in C, ctypes and Rust."""
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
    assert C.sizeof(_lib.CCorrectCounts) == 32
    src = tmp_path / "s.c"
    src.write_text('#include "ibu_hip.h"\n_Static_assert(sizeof(ibu_correct_counts_t) == 32, "four u64");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    m = re.search(r"#\[repr\(C\)\][^{]*?pub struct ibu_correct_counts_t\s*\{(.*?)\n\}", ffi, flags=re.S)
    assert m, "ffi.rs has no #[repr(C)] ibu_correct_counts_t"
    fields = [f.split(":")[1].strip() for f in m.group(1).split(",") if ":" in f]
    assert fields == ["u64"] * 4, fields
    import ibu_amd
    assert hasattr(ibu_amd, "Whitelist") and hasattr(ibu_amd.Context, "correct_barcodes") and hasattr(ibu_amd.Context, "select_records")
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub struct Whitelist" in lib_rs and re.search(r"impl Drop for Whitelist", lib_rs)
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    assert "class Whitelist" in hpp and "correct_barcodes" in hpp and "select_records" in hpp


def test_whitelist_fails_loudly_without_gpu():
    """No device: NoDevice from the library — there is no host form of the correction to fall back to."""
    import ibu_amd
    if ibu_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Whitelist(None, 0, 1, 16)
    assert ei.value.kind == "NoDevice"
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Whitelist.from_ascii(ibu_amd.Context(0), ["ACGT"])
    assert ei.value.kind == "NoDevice"


def test_correct_file_example_compiles(tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "correct_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "correct_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: correct_file" in r.stderr
