"""Whitelist abundance and the resolution of ambiguous barcodes — what can be checked without a GPU: the numpy statement of the
semantics (tests/resolve_np.py) against brute force with Python dicts and a Hamming loop, the premise that a legal share names
at most one winner, the crafted cases of tests/test_gpu_resolve.py, the new entry points in every layer of the ABI, and the loud
failure on a box without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import resolve_np as rnp
from tests import whitelist_np as wnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_abundance_create", "ibu_abundance_reset", "ibu_abundance_info", "ibu_abundance_destroy", "ibu_abundance_add",
         "ibu_abundance_counts", "ibu_resolve_barcodes")
LEGAL = rnp.SHARES + [(2, 3), (51, 100), (5, 9), ((1 << 23), (1 << 24) - 1)]


def _brute_chain(wl, bc_len, bc, num, den, class_mask=1):
    cls, out = wnp.brute_force(bc, wl, bc_len, 1)
    table = rnp.brute_add({}, wl, bc_len, out, cls, class_mask)
    return rnp.brute_resolve(table, wl, bc_len, out, cls, num, den), table


@pytest.mark.parametrize("bc_len,w,n", [(5, 200, 3000), (16, 300, 3000), (32, 300, 2000)])
def test_numpy_statement_equals_brute_force(bc_len, w, n):
    rng = np.random.default_rng(0x1B00900 + bc_len)
    wl, bc = rnp.make_case(rng, bc_len, w, n)
    recs = rnp.records(rng, bc)
    if bc_len < 32:
        assert (bc >> np.uint64(2 * bc_len)).any(), "junk bits above 2*bc_len are part of the input"
    seen = set()
    for num, den in LEGAL:
        for class_mask in (0b0001, 0b0011):
            out, cls, tot, ab = rnp.chain(wl, bc_len, recs, num, den, class_mask)
            (out_b, cls_b, tot_b, most), table = _brute_chain(wl, bc_len, bc, num, den, class_mask)
            assert (out["barcode"] == out_b).all() and (cls == cls_b).all() and tot == tot_b, (num, den, class_mask)
            assert most <= 1, "two candidates of one record pass a share above one half"
            assert rnp.counts(ab, ab.wl).tolist() == [table.get(int(c), 0) for c in ab.wl]
            assert tot["examined"] == tot["resolved"] + tot["below_share"] + tot["unseen"]
            # what resolve may touch: the low bits and the class byte of the records it resolves
            _, cls0, _ = wnp.correct_records(recs, wl, bc_len, 1)
            want0 = wnp.correct_records(recs, wl, bc_len, 1)[0]
            moved = cls == rnp.RESOLVED
            assert (cls0[moved] == 2).all() and (cls[~moved] == cls0[~moved]).all() and out[~moved].tobytes() == want0[~moved].tobytes()
            m = wnp.mask(bc_len)
            assert (out["umi"] == recs["umi"]).all() and (out["index"] == recs["index"]).all()
            assert bc_len == 32 or ((out["barcode"] & ~m) == (recs["barcode"] & ~m)).all()
            assert np.isin(out["barcode"][moved] & m if bc_len < 32 else out["barcode"][moved], wl).all()
            # a second resolve finds nothing it could change
            again, cls_again, tot_again = rnp.resolve(ab, out, cls, num, den)
            assert again.tobytes() == out.tobytes() and (cls_again == cls).all() and tot_again["resolved"] == 0
            if (num, den) == (39, 40) and class_mask == 1:
                print(bc_len, w, n, tot)
                seen = {k for k in rnp.TOTALS if tot[k]}
    # (in a whitelist of 200 of the 1024 five-base codes every barcode has some forty whitelisted neighbours: none is `unseen`)
    assert seen >= set(rnp.TOTALS) - ({"unseen"} if bc_len == 5 else set()), f"the default share leaves an outcome unexercised: {seen}"


def test_add_and_counts_statement():
    ab = rnp.Abundance([5, 9, 9, 1 << 19], 10)
    bc = np.array([5, 5, 9, 6, 5 | (7 << 20), 1 << 19, 12], np.uint64)
    cls = np.array([0, 1, 0, 3, 0, 9, 2], np.uint8)
    assert rnp.counts(rnp.add(ab.copy(), bc), [5, 9, 1 << 19, 6, 5 | (1 << 20)]).tolist() == [3, 1, 1, 0, 0]       # junk bits: add ignores them, counts does not
    assert rnp.counts(rnp.add(ab.copy(), bc, cls, 0b0001), [5, 9, 1 << 19]).tolist() == [2, 1, 0]
    assert rnp.counts(rnp.add(ab.copy(), bc, cls, 0b0011), [5, 9, 1 << 19]).tolist() == [3, 1, 0]
    assert rnp.counts(rnp.add(ab.copy(), bc, cls, 0), [5, 9, 1 << 19]).tolist() == [0, 0, 0]
    assert rnp.counts(rnp.add(ab.copy(), bc, cls, 0xFFFFFFFF), [5, 9, 1 << 19]).tolist() == [3, 1, 0]              # class 9 never counts
    twice = rnp.add(rnp.add(ab.copy(), bc[:3]), bc[3:])
    assert (twice.n == rnp.add(ab.copy(), bc).n).all() and (rnp.add(ab.copy(), bc, times=3).n == 3 * rnp.add(ab.copy(), bc).n).all()
    table = rnp.brute_add({}, [5, 9, 1 << 19], 10, bc, cls, 0b0011)
    assert table == {5: 3, 9: 1}
    twice.reset()
    assert not twice.n.any()


def test_share_arguments():
    for num, den in LEGAL:
        assert rnp.legal_share(num, den)
    for num, den in ((1, 2), (2, 4), (0, 1), (3, 2), (1, 0), (0, 0), (1 << 24, 1 << 24), (1 << 23, 1 << 24), (20, 40)):
        assert not rnp.legal_share(num, den), (num, den)
        with pytest.raises(ValueError):
            rnp.resolve(rnp.Abundance([1], 4), np.zeros(1, rnp.REC), np.zeros(1, np.uint8), num, den)


@pytest.mark.parametrize("num,den", rnp.SHARES)
@pytest.mark.parametrize("bc_len", [12, 16, 32])
def test_boundary_cases_are_what_they_claim(bc_len, num, den):
    """Counters set exactly around best * den == num * total: the numpy statement and brute force give the planned outcome."""
    wl, setc, mids, outcome, low = rnp.boundary_case(bc_len, num, den)
    assert len(np.unique(wl)) == len(wl) and not np.isin(mids, wl).any()
    cls0, _ = wnp.classify(mids, wl, bc_len, 1)
    assert (cls0 == 2).all()
    ab = rnp.Abundance(wl, bc_len)
    for code, k in setc:
        ab.n[np.searchsorted(ab.wl, np.uint64(code))] += np.uint64(k)
    recs = rnp.records(np.random.default_rng(1), mids)
    out, cls, tot = rnp.resolve(ab, recs, cls0, num, den)
    assert [("resolved" if c == rnp.RESOLVED else "unseen" if o == "unseen" else "below_share") for c, o in zip(cls, outcome)] == outcome
    assert (out["barcode"] == low).all()
    assert tot == {"examined": len(mids), **{k: outcome.count(k) for k in rnp.TOTALS[1:]}}
    out_b, cls_b, tot_b, most = rnp.brute_resolve({int(c): int(k) for c, k in setc}, wl, bc_len, mids, cls0, num, den)
    assert (out_b == low).all() and (cls_b == cls).all() and tot_b == tot and most == 1
    specs = rnp.boundary_counts(num, den)
    g = np.gcd(num, den)
    assert specs[0][0][0] * den == num * sum(specs[0][0]) and sum(specs[0][0]) == den // g, "the first case sits exactly on the boundary"
    assert {"resolved", "unseen"} <= set(outcome) and (num == den or "below_share" in outcome)
    assert any(len(s[0]) == 3 for s in specs)


@pytest.mark.parametrize("bc_len", [16, 22, 23, 32])
def test_seam_cases_are_what_they_claim(bc_len):
    wl, bc, low, mids = rnp.seam_case(bc_len)
    recs = rnp.records(np.random.default_rng(2), bc)
    out, cls, tot, ab = rnp.chain(wl, bc_len, recs)
    at = {int(b): k for k, b in enumerate(bc)}
    rows = np.array([at[int(c)] for c in mids])
    assert (cls[rows] == rnp.RESOLVED).all() and (out["barcode"][rows] == low).all()
    assert tot == {"examined": len(mids), "resolved": len(mids), "below_share": 0, "unseen": 0}
    (out_b, cls_b, tot_b, most), _ = _brute_chain(wl, bc_len, bc, 39, 40)
    assert (out_b == out["barcode"]).all() and (cls_b == cls).all() and tot_b == tot and most == 1
    # where the winner sits among the neighbours of its midpoint, as the device counts them
    nn = 3 * bc_len
    where = [[j for j in range(nn) if wnp.neighbour(c, j) == int(v)][0] for c, v in zip(mids, low)]
    rivals = []
    for c, v in zip(mids, low):
        near = [j for j in range(nn) if np.uint64(wnp.neighbour(c, j)) in wl and wnp.neighbour(c, j) != int(v)]
        assert len(near) == 1
        rivals.append(near[0])
    kinds = {(a < 64, b < 64, a < b) for a, b in zip(where, rivals)}
    assert {(True, True, True), (True, True, False)} <= kinds                      # both in the first ballot, winner first / second
    if bc_len >= 22:
        assert {(True, False, True), (False, True, False)} <= kinds                # one on each side of the seam
    if bc_len >= 23:
        assert {(False, False, True), (False, False, False)} <= kinds              # both in the second ballot
    if bc_len == 32:
        ones = np.uint64(wnp.FREE)
        assert ones in wl and (low == ones).sum() == 4 and rnp.counts(ab, [ones]).tolist() == [50]
        def ones_at(c):
            js = [j for j in range(nn) if wnp.neighbour(c, j) == wnp.FREE]
            return js[0] if js else None

        assert {ones_at(c) for c, v in zip(mids, low) if v == ones} == {0, 63, 64, 95}                                  # all ones wins
        assert {ones_at(c) for c, v in zip(mids, low) if v != ones and ones_at(c) is not None} == {2, 65, 66, 93}      # ... and loses

def test_entry_points_exist_in_every_layer(tmp_path):
    """Header, shared library, ctypes table, Rust extern block, the C++ mirror; ibu_resolve_counts_t is 32 bytes in C, ctypes and Rust."""
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
    assert re.search(r"#define\s+IBU_BARCODE_RESOLVED\s+4\b", code)
    assert C.sizeof(_lib.CResolveCounts) == 32
    src = tmp_path / "s.c"
    src.write_text('#include "ibu_hip.h"\n_Static_assert(sizeof(ibu_resolve_counts_t) == 32, "four u64");\n'
                   '_Static_assert(IBU_BARCODE_RESOLVED == 4, "the class after 0..3");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    m = re.search(r"#\[repr\(C\)\][^{]*?pub struct ibu_resolve_counts_t\s*\{(.*?)\n\}", ffi, flags=re.S)
    assert m, "ffi.rs has no #[repr(C)] ibu_resolve_counts_t"
    fields = [f.split(":")[0].replace("pub", "").strip() for f in m.group(1).split(",") if ":" in f]
    assert fields == list(rnp.TOTALS), fields
    assert [f for f, _ in _lib.CResolveCounts._fields_] == list(rnp.TOTALS)
    import ibu_amd
    assert ibu_amd.BARCODE_RESOLVED == rnp.RESOLVED == 4
    assert hasattr(ibu_amd, "Abundance") and hasattr(ibu_amd.Whitelist, "abundance") and hasattr(ibu_amd.Context, "resolve_barcodes")
    for method in ("add", "counts", "reset", "close"):
        assert hasattr(ibu_amd.Abundance, method)
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub struct Abundance" in lib_rs and re.search(r"impl Drop for Abundance", lib_rs) and "pub fn resolve_barcodes" in lib_rs
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    assert "class Abundance" in hpp and "resolve_barcodes" in hpp


def test_abi_revision_is_unchanged():
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "new entry points change no signature"


def test_fails_loudly_without_gpu():
    """No device: NoDevice from the library — there is no host form of the counters or of the resolution to fall back to."""
    import ibu_amd
    if ibu_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Abundance(None, None)
    assert ei.value.kind == "NoDevice"
    so = ibu_amd.lib
    h = C.c_void_p()
    rc = so.ibu_abundance_create(None, None, None, C.byref(h))
    assert so.ibu_status_name(rc) == b"NoDevice" and not h.value
    # the calls that work on a context refuse a NULL one before they look at anything else
    for rc in (so.ibu_abundance_add(None, None, None, None, 0, 1, None), so.ibu_abundance_counts(None, None, None, 0, None, None),
               so.ibu_resolve_barcodes(None, None, None, None, 0, 39, 40, None, None, None)):
        assert rc != 0 and so.ibu_status_name(rc) == b"InvalidArg"
    assert so.ibu_abundance_reset(None, None) != 0 and so.ibu_abundance_info(None, None) != 0
    so.ibu_abundance_destroy(None)


def test_correct_file_example_knows_resolve(tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "correct_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "correct_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "--resolve[=NUM/DEN]" in r.stderr
    r = subprocess.run([str(exe), "in", "wl", "out", "--resolve=39"], capture_output=True, text=True)
    assert r.returncode == 2 and "NUM/DEN" in r.stderr
