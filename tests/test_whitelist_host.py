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


# ---- the table model and the crafted cases of tests/test_gpu_whitelist_edges.py: their premises, asserted without a GPU ----
def test_table_model_assumes_the_hash_the_kernel_has():
    """Tripwire: the crafted cases rest on the multiplier and the 1024-slot minimum of ibu_amd/csrc/k_whitelist.hip.  If this
    fails the hash or the table size changed: the GPU comparisons stay valid (classify() knows no tables), but the crafted
    whitelists no longer form the clusters they were made for; bring whitelist_np.PHI / MIN_SLOTS / table_slots() along."""
    src = open(os.path.join(ROOT, "ibu_amd", "csrc", "k_whitelist.hip")).read()
    m = re.search(r"u32 wl_slot\(u64 key, u32 shift\)\s*\{[^}]*?return \(u32\)\(\(key \* (0x[0-9A-Fa-f]+)ull\) >> shift\);", src)
    assert m and int(m.group(1), 16) == wnp.PHI, "wl_slot no longer is (key * PHI) >> shift"
    m = re.search(r"size_t whitelist_slots\(size_t w\)\s*\{[^}]*?size_t s = (\d+);\s*while \(s < 2 \* w\) s <<= 1;", src)
    assert m and int(m.group(1)) == wnp.MIN_SLOTS, "whitelist_slots no longer is the power of two >= max(1024, 2 w)"
    assert re.search(r"static constexpr u64 kEmpty = ~0ull;", src) and wnp.FREE == 2 ** 64 - 1
    assert re.search(r"s = \(s \+ 1\) & mask;", src), "the probe sequence no longer is linear"
    assert wnp.PHI * wnp.PHI_INV % 2 ** 64 == 1
    assert [wnp.table_slots(w) for w in (1, 2, 512, 513, 1000, 1024, 1025, 100_000)] == [1024, 1024, 1024, 2048, 2048, 2048, 4096, 262_144]


def test_table_model_by_hand():
    slots, homes, table = wnp.table_model([5, 5, 7], 16)
    assert slots == 1024 and homes.tolist() == [(k * wnp.PHI % 2 ** 64) >> 54 for k in (5, 5, 7)]
    assert sorted(table[table != np.uint64(wnp.FREE)].tolist()) == [5, 7] and table[homes[0]] == 5 and table[homes[2]] == 7
    with pytest.raises(ValueError):
        wnp.table_model([1 << 20], 10)
    slots, homes, table = wnp.table_model([wnp.FREE, 3], 32)          # all ones is a code at 32 bases and stays out of the table
    assert (table != np.uint64(wnp.FREE)).sum() == 1
    t = np.full(16, wnp.FREE, np.uint64)
    t[[14, 15, 0, 1, 2, 7, 8]] = 1
    assert wnp.clusters(t) == [(14, 5), (7, 2)]
    # the taken slots do not depend on the order of insertion, the key in a slot does
    rng = np.random.default_rng(1)
    keys = wnp.craft_keys(rng, 16, 1024, [7, 8], 40)
    t1, t2 = wnp.table_model(keys, 16)[2], wnp.table_model(keys[::-1], 16)[2]
    assert ((t1 == np.uint64(wnp.FREE)) == (t2 == np.uint64(wnp.FREE))).all() and (t1 != t2).any()
    assert wnp.clusters(t1) == [(7, 40)]
    steps = wnp.probe_lengths(t1, keys)
    assert (t1[(wnp.home_slots(keys, 1024) + steps - 1) % 1024] == keys).all() and steps.min() == 1 and 20 <= steps.max() <= 40
    assert wnp.probe_lengths(t1, [12345]).tolist() == [1 if not 7 <= h < 47 else 48 - h for h in wnp.home_slots([12345], 1024).tolist()]


@pytest.mark.parametrize("bc_len", [10, 16, 31, 32])
def test_craft_keys_against_the_model(bc_len):
    rng = np.random.default_rng(bc_len)
    big = [(1 << 18, [5, 1 << 17], 50)] if bc_len > 10 else []    # (the 4^10 ten-base codes come to four per slot of such a table)
    for slots, homes, count in [(1024, [0], 100), (1024, [1023, 3], 700), (2048, [2047], 300)] + big:
        keys = wnp.craft_keys(rng, bc_len, slots, homes, count)
        assert len(np.unique(keys)) == count and not (keys == np.uint64(wnp.FREE)).any()
        assert bc_len == 32 or not (keys >> np.uint64(2 * bc_len)).any()
        shift = 64 - (slots.bit_length() - 1)
        assert {(int(k) * wnp.PHI % 2 ** 64) >> shift for k in keys} == set(homes)       # Python integers, not numpy's wrap-around
        more = wnp.craft_keys(rng, bc_len, slots, homes, 20, exclude=keys)
        assert not np.isin(more, keys).any()
    with pytest.raises(ValueError):
        wnp.craft_keys(rng, 4, 1024, [0], 2)                     # the 256 four-base codes have 256 of the 1024 home slots


@pytest.mark.parametrize("tripled", [False, True])
@pytest.mark.parametrize("kind", sorted(wnp.CRAFTED_TABLES))
@pytest.mark.parametrize("bc_len", [10, 16, 31, 32])
def test_crafted_tables_are_what_they_claim(bc_len, kind, tripled):
    """One cluster that holds every key, starts at the keys' first home slot and runs through the last slot into slot 0; at a
    load of exactly 1/2 for the two chains; every walker reads the chain to the free slot behind it; brute force agrees with
    classify() on a prefix that has every kind of barcode."""
    slots0, homes0, w = wnp.CRAFTED_TABLES[kind]
    wl, keys, walkers, bc = wnp.crafted_table_case(bc_len, kind, tripled, 3000)
    assert len(np.unique(keys)) == w and len(wl) == (3 * w if tripled else w) and (np.unique(wl) == np.unique(keys)).all()
    slots, homes, table = wnp.table_model(wl, bc_len)
    assert slots == wnp.table_slots(len(wl)) == ((2 if kind == "wrap300" else 4) if tripled else 1) * slots0
    assert kind == "wrap300" or 2 * w == slots0                                       # load exactly 1/2 where the keys come once
    scale = slots // slots0
    assert set((homes // scale).tolist()) == set(homes0)
    (start, length), = wnp.clusters(table)                                            # one cluster
    assert length == w and start == homes.min() >= slots - scale * len(homes0) and start + length > slots, (start, length)
    assert not np.isin(walkers, keys).any()
    steps = wnp.probe_lengths(table, walkers)
    assert steps.min() >= w - wnp.WALKER_HOMES + 1 and steps.max() <= w + 1
    assert wnp.probe_lengths(table, keys).max() >= w // (scale * len(homes0))           # the last key of the fullest home slot
    cls, out = wnp.classify(bc, wl, bc_len, 1)
    cls_b, out_b = wnp.brute_force(bc, wl, bc_len, 1)
    assert (cls == cls_b).all() and (out == out_b).all()
    low = bc & wnp.mask(bc_len)
    assert np.isin(low, keys).sum() >= 700 and np.isin(low, walkers).sum() >= 700 and (cls == 1).sum() >= 700 and (cls == 3).sum() >= 700
    assert bc_len == 32 or (bc >> np.uint64(2 * bc_len)).any()


def _bases_apart(a, b):
    d = int(a) ^ int(b)
    return bin((d | (d >> 1)) & 0x5555555555555555).count("1")


@pytest.mark.parametrize("bc_len,with_ones", [(21, True), (22, True), (23, True), (31, True), (32, True), (32, False)])
def test_ballot_cases_are_what_they_claim(bc_len, with_ones):
    wl, bc, cls, low, specs = wnp.ballot_case(bc_len, with_ones)
    got, out = wnp.classify(bc, wl, bc_len, 1)
    got_b, out_b = wnp.brute_force(bc, wl, bc_len, 1)
    assert (got == cls).all() and (got_b == cls).all() and (out == low).all() and (out_b == low).all()
    assert set(cls.tolist()) == {0, 1, 2, 3}
    plain = [s for s in specs if s[0] != "ones"]
    for spec, c, b in zip(plain, cls, bc):                       # the planted neighbours are where the spec says
        assert c == (1 if len(spec) == 1 else 2)
        assert sorted(wnp.neighbour(b, j) for j in spec) == sorted(int(e) for e in wl if _bases_apart(e, b) == 1)
    pairs = [s for s in plain if len(s) == 2]
    singles = {s[0] for s in plain if len(s) == 1}
    assert {0, 62, 3 * bc_len - 1} <= singles and any(max(s) < 64 for s in pairs)
    if bc_len >= 22:                                             # a second ballot exists
        assert {63, 64, 65} <= singles
        assert any(min(s) >= 64 for s in pairs) and any(min(s) < 64 <= max(s) for s in pairs) and (63, 64) in pairs
    if bc_len >= 23:
        assert any(min(s) >= 66 for s in pairs), "a pair with both bases at or above 22"
        assert any(min(s) >= 66 and s[0] // 3 == s[1] // 3 for s in pairs)
    if bc_len == 32:
        ones = [(s, int(c), int(v)) for s, c, v in zip(specs[len(plain):], cls[len(plain) + 2:], low[len(plain) + 2:])]   # (+ 2: the exact and the lone centre)
        assert [s[1] for s, _, _ in ones[:4]] == [0, 63, 64, 95]
        if with_ones:
            assert np.uint64(wnp.FREE) in wl and all(c == 1 and v == wnp.FREE for _, c, v in ones[:4]) and all(c == 2 for _, c, _ in ones[4:])
        else:
            assert np.uint64(wnp.FREE) not in wl and all(c == 3 for _, c, _ in ones[:4]) and all(c == 1 and v != wnp.FREE for _, c, v in ones[4:])


def test_miss_case_has_no_exact_barcode_and_every_other_class():
    wl, pools = wnp.miss_case()
    for c in (1, 2, 3):
        assert len(pools[c]) >= 64, (c, len(pools[c]))
        got, _ = wnp.classify(pools[c], wl, 16, 1)
        assert (got == c).all() and (wnp.brute_force(pools[c][:200], wl, 16, 1)[0] == c).all()
        assert set(wnp.classify(pools[c], wl, 16, 0)[0].tolist()) == {3}
