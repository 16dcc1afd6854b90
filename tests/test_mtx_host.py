"""The matrix export (ibu_matrix_rows, ibu_matrix_market_body) — what can be checked without a GPU: the numpy / Python statement of the
semantics (tests/mtx_np.py) against cases a reader can check by eye, the text it makes read back to the triples it was made from, the
digit arithmetic of ibu_amd/csrc/dec_format.hpp against snprintf in a stand-alone C++ program (built plain and with the address and
undefined-behaviour sanitizers: host code, its own main, nothing loaded into Python), and the entry points in every layer of the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mtx_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibu_matrix_rows", "ibu_matrix_market_body")
A, B = 7, 1 << 63


def _u64(xs):
    return np.array(xs, np.uint64)


# ---- the statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,ordinals,keys,ptr", [
    ([], [], [], [0]),
    ([A], [0], [A], [0, 1]),
    ([A, A, A], [0, 0, 0], [A], [0, 3]),
    ([A, B, A], [0, 1, 2], [A, B, A], [0, 1, 2, 3]),             # equal keys in runs that are not adjacent: three rows
    ([A, A, B, B, B, A], [0, 0, 1, 1, 1, 2], [A, B, A], [0, 2, 5, 6]),
    ([0, 0, 1, 2, 2], [0, 0, 1, 2, 2], [0, 1, 2], [0, 2, 3, 5]),
])
def test_matrix_rows_by_hand(first, ordinals, keys, ptr):
    got = mtx_np.matrix_rows(_u64(first))
    assert [g.dtype for g in got] == [np.uint64] * 3
    assert [g.tolist() for g in got] == [ordinals, keys, ptr]


def test_matrix_rows_is_the_csr_of_a_run_length_encoding():
    rng = np.random.default_rng(0x3A7100)
    for _ in range(200):
        lens = rng.integers(1, 6, int(rng.integers(0, 30)))
        keys = (np.cumsum(rng.integers(1, 3, len(lens))) % 3).astype(np.uint64)   # neighbours differ, values repeat further on
        assert len(keys) < 2 or (keys[1:] != keys[:-1]).all()
        ordinals, got_keys, ptr = mtx_np.matrix_rows(np.repeat(keys, lens))
        assert got_keys.tolist() == keys.tolist() and np.diff(ptr.astype(np.int64)).tolist() == lens.tolist()
        assert ordinals.tolist() == np.repeat(np.arange(len(lens)), lens).tolist()


@pytest.mark.parametrize("cols,add,text,maxima", [
    (([], [], []), (1, 1), b"", (0, 0, 0)),
    (([0], [0], [0]), (0, 0), b"0 0 0\n", (0, 0, 0)),
    (([0], [0], [0]), (1, 1), b"1 1 0\n", (1, 1, 0)),
    (([9, 99], [10, 0], [5, 12345678901234567890]), (1, 1), b"10 11 5\n100 1 12345678901234567890\n", (100, 11, 12345678901234567890)),
    (([(1 << 64) - 1], [(1 << 64) - 1], [(1 << 64) - 1]), (1, 0), b"0 18446744073709551615 18446744073709551615\n",
     (0, (1 << 64) - 1, (1 << 64) - 1)),                         # the sum wraps; the value column takes no addend
    (([(1 << 64) - 2] * 3, [3] * 3, [1, 2, 3]), (3, (1 << 64) - 3), b"1 0 1\n1 0 2\n1 0 3\n", (1, 0, 3)),
])
def test_body_by_hand(cols, add, text, maxima):
    assert mtx_np.body(*cols, *add) == (text, maxima)


def test_line_lengths_are_6_to_63():
    top = (1 << 64) - 1
    assert len(mtx_np.body([0], [0], [0], 0, 0)[0]) == 6 and len(mtx_np.body([top], [top], [top], 0, 0)[0]) == 63


def test_body_reads_back_to_its_triples(tmp_path):
    rng = np.random.default_rng(0x3A7200)
    n_features, n_rows = 40, 17
    rows = np.sort(rng.integers(0, n_rows, 300)).astype(np.uint64)
    feats = rng.integers(0, n_features, 300).astype(np.uint64)
    vals = rng.integers(1, 1 << 40, 300).astype(np.uint64)
    text, maxima = mtx_np.body(feats, rows, vals, 1, 1)
    assert maxima == (int(feats.max()) + 1, int(rows.max()) + 1, int(vals.max()))
    (tmp_path / "matrix.mtx").write_bytes(f"{mtx_np.BANNER}\n{n_features} {n_rows} 300\n".encode() + text)
    (tmp_path / "barcodes.tsv").write_text("".join(f"BC{r}-1\n" for r in range(n_rows)))
    (tmp_path / "features.tsv").write_text("".join(f"{j}\t{j}\tGene Expression\n" for j in range(n_features)))
    nf, barcodes, features, coo = mtx_np.read_directory(str(tmp_path))
    assert nf == n_features and barcodes[3] == "BC3-1" and features == [str(j) for j in range(n_features)]
    assert coo == [(f"BC{int(r)}-1", int(f), int(v)) for f, r, v in zip(feats, rows, vals)]


# ---- the digit arithmetic ----------------------------------------------------------------------------------------------
DEC_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dec_format.hpp"

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static unsigned long long next() {   // splitmix64
  unsigned long long z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static long checked = 0;
static int check(unsigned long long v) {
  char want[32], got[32];
  const int n = snprintf(want, sizeof want, "%llu", v);
  const uint32_t nd = ibu::dec_digits(v);
  if ((int)nd != n) { printf("digits of %llu: %u, snprintf %d\n", v, nd, n); return 1; }
  if (v <= 0xFFFFFFFFull && (int)ibu::dec_digits32((uint32_t)v) != n) { printf("32-bit digits of %llu, snprintf %d\n", v, n); return 1; }
  memset(got, '#', sizeof got);
  unsigned calls = 0;
  ibu::dec_emit(v, nd, [&](uint32_t k, char c) { if (k < nd) got[nd - 1 - k] = c; ++calls; });
  got[nd] = 0;
  if (calls != nd || strcmp(want, got)) { printf("text of %llu: %s in %u calls\n", v, got, calls); return 1; }
  uint32_t lo, mid, hi;
  ibu::dec_chunks(v, lo, mid, hi);
  if (lo >= 1000000000u || mid >= 1000000000u || hi > 18 || ((unsigned long long)hi * 1000000000ull + mid) * 1000000000ull + lo != v) {
    printf("chunks of %llu: %u %u %u\n", v, hi, mid, lo);
    return 1;
  }
  ++checked;
  return 0;
}
int main() {
  int bad = check(0);
  unsigned long long p = 1;
  for (int k = 1; k <= 19; ++k) {
    p *= 10;
    bad |= check(p - 1) | check(p);
  }
  bad |= check(0xFFFFFFFFull) | check(0x100000000ull) | check(1ull << 63) | check(~0ull);
  for (unsigned x = 0; x < 200000u; x += 7) bad |= ibu::dec_div10(x) != x / 10;
  for (unsigned x = 0xFFFFFFFFu; x > 0xFFFFFFFFu - 1000u; --x) bad |= ibu::dec_div10(x) != x / 10;
  // 1e5 values spread over all digit counts: a random value cut down to a random number of digits 1 .. 20
  unsigned long long pow10[20];
  pow10[0] = 1;
  for (int k = 1; k < 20; ++k) pow10[k] = pow10[k - 1] * 10;
  int seen[21] = {0};
  for (int i = 0; i < 100000 && !bad; ++i) {
    const int d = 1 + (int)(next() % 20);
    unsigned long long v = next();
    if (d == 1) v %= 10;
    else if (d < 20) v = pow10[d - 1] + v % (pow10[d] - pow10[d - 1]);
    else v = pow10[19] + v % (~0ull - pow10[19] + 1);
    seen[ibu::dec_digits(v)]++;
    bad |= check(v);
  }
  for (int d = 1; d <= 20; ++d)
    if (seen[d] < 1000) { printf("only %d values of %d digits\n", seen[d], d); bad = 1; }
  printf("%s %ld\n", bad ? "BAD" : "OK", checked);
  return bad;
}
"""


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_dec_format_against_snprintf(tmp_path, flags):
    src = tmp_path / "dec_main.cpp"
    src.write_text(DEC_MAIN)
    exe = tmp_path / "dec_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "ibu_amd", "csrc"),
                           str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["OK", str(1 + 38 + 4 + 100000)], r.stdout[-2000:] + r.stderr[-2000:]


# ---- the layers --------------------------------------------------------------------------------------------------------
def test_every_layer_declares_the_entry_points():
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert hasattr(so, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ibu_matrix_rows"][1]) == 9 and len(_lib.SIGNATURES["ibu_matrix_market_body"][1]) == 12
    texts = {p: open(os.path.join(ROOT, *p.split("/"))).read()
             for p in ("include/ibu_hip.h", "include/ibu.hpp", "bindings/rust/src/ffi.rs", "bindings/rust/src/lib.rs", "ibu_amd/csrc/kernels.h")}
    for name in NAMES:
        for p in ("include/ibu_hip.h", "include/ibu.hpp", "bindings/rust/src/ffi.rs", "bindings/rust/src/lib.rs"):
            assert name in texts[p], (name, p)
    assert "need nothing new" not in texts["include/ibu_hip.h"]
    import ibu_amd
    for method in ("matrix_rows", "matrix_market_body", "matrix_csr", "write_matrix_market"):
        assert callable(getattr(ibu_amd.Context, method))


def test_kernels_are_in_the_library_and_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = kernel_resources.all_kernels(_lib.SO_PATH)
    mine = {k: v for k, v in ks.items() if k.startswith("ibu_k_matrix_")}
    assert sorted(mine) == ["ibu_k_matrix_rows_count", "ibu_k_matrix_rows_scatter", "ibu_k_matrix_scan", "ibu_k_matrix_text_count",
                            "ibu_k_matrix_text_write"]
    assert all(v.get("private_segment_fixed_size", 0) == 0 and not v.get("uses_dynamic_stack", 0) for v in mine.values()), mine
    assert mine["ibu_k_matrix_text_write"]["group_segment_fixed_size"] == 16384   # 4 KiB of stage per wave
    assert "ibu_k_select_scan" in ks                                            # select keeps its own entry point
