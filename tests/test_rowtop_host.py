"""The per-row top-2 and the row class (ibu_matrix_row_top, ibu_assign_rows) — what can be checked without a GPU: the numpy / Python
statement of the semantics (tests/rowtop_np.py) against a brute-force loop over the rows and against cases a reader can check by
eye, and the entry points in every layer of the ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rowtop_np as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ibu_matrix_row_top": 15, "ibu_assign_rows": 9}        # the argument counts of include/ibu_hip.h
M64 = (1 << 64) - 1


def _u64(xs):
    return np.array(xs, np.uint64)


# ---- the statement -----------------------------------------------------------------------------------------------------
def _brute(first, second, values, set_words, set_bits):
    """One row at a time, one entry at a time, in Python integers."""
    rows, k, n = [], 0, len(first)
    while k < n:
        e = k
        while e < n and first[e] == first[k]:
            e += 1
        best, best_at, total, entries, taking = -1, None, 0, 0, []
        for j in range(k, e):
            s = second[j]
            if set_words is not None and not (s < set_bits and (int(set_words[s >> 6]) >> (s & 63)) & 1):
                continue
            taking.append(j)
            total += values[j]
            entries += 1
            if values[j] > best:                                 # strictly: the first entry with the largest value stays
                best, best_at = values[j], j
        if best_at is None:
            rows.append((rt.NO_KEY, 0, 0, 0, 0))
        else:
            others = [values[j] for j in taking if j != best_at]
            rows.append((second[best_at], best, max(others) if others else 0, total & M64, entries))
        k = e
    return rows


def _random_table(rng):
    n = int(rng.integers(0, 60))
    lens = rng.integers(1, 9, n + 1)
    first = np.repeat(rng.integers(0, 3, n + 1).astype(np.uint64) << np.uint64(62), lens)[:n]   # neighbours may be equal: runs merge
    set_bits = int(rng.choice([0, 1, 5, 64, 65, 200]))
    special = [max(set_bits - 1, 0), set_bits, (1 << 32) + 3, (1 << 32) + int(rng.integers(0, 64)), 0, 3, 63, 64, M64]
    second = _u64([special[i] for i in rng.integers(0, len(special), n)])
    kind = int(rng.integers(0, 4))
    if kind == 0:
        values = rng.integers(0, 4, n).astype(np.uint64)         # ties and zeros
    elif kind == 1:
        values = np.zeros(n, np.uint64)
    elif kind == 2:
        values = _u64([[M64, 1 << 63, 0, 1][i] for i in rng.integers(0, 4, n)])   # sums wrap
    else:
        values = rng.integers(0, 1 << 62, n).astype(np.uint64)
    if rng.random() < 0.25:
        return first, second, values, None, 0
    chosen = [v for v in range(set_bits) if rng.random() < 0.6]
    return first, second, values, rt.bitmap(chosen, set_bits), set_bits


def test_row_top_against_a_loop_over_the_rows():
    rng = np.random.default_rng(0x70B200)
    seen = {"empty_row": 0, "tie": 0, "wrap": 0, "alias": 0, "edge": 0}
    for _ in range(400):
        first, second, values, words, bits = _random_table(rng)
        got = rt.row_top(first, second, values, words, bits)
        assert [g.dtype for g in got] == [np.uint64] * 5
        want = _brute(first.tolist(), second.tolist(), values.tolist(), words, bits)
        assert list(zip(*[g.tolist() for g in got])) == want
        part = rt.takes_part(second, words, bits)
        if words is not None:
            assert not part[second >= np.uint64(bits)].any()      # a key of set_bits or more never takes part
            seen["alias"] += int(((second >= np.uint64(1 << 32)) & (second < np.uint64(1 << 33))).any())
            seen["edge"] += int(bits > 0 and (second == np.uint64(bits - 1)).any() and (second == np.uint64(bits)).any())
        for key, top, nxt, total, entries in want:
            seen["empty_row"] += entries == 0
            seen["tie"] += entries >= 2 and top == nxt
        seen["wrap"] += int(sum(values.tolist()) > M64)
    assert all(v >= 10 for v in seen.values()), seen


@pytest.mark.parametrize("first,second,values,chosen,bits,want", [
    ([], [], [], None, 0, []),
    ([7], [3], [9], None, 0, [(3, 9, 0, 9, 1)]),
    ([7, 7, 7], [1, 2, 3], [5, 5, 5], None, 0, [(1, 5, 5, 15, 3)]),                 # tied: the first entry, next == top
    ([7, 7, 8, 7], [1, 2, 1, 2], [1, 4, 0, 2], None, 0, [(2, 4, 1, 5, 2), (1, 0, 0, 0, 1), (2, 2, 0, 2, 1)]),   # A, B, A: three rows
    ([7, 7, 7], [0, 1, 2], [9, 4, 6], [1, 2], 3, [(2, 6, 4, 10, 2)]),                # the set leaves the maximum out
    ([7, 7], [3, (1 << 32) + 1], [9, 4], [1], 3, [(rt.NO_KEY, 0, 0, 0, 0)]),         # 3 >= set_bits; 2^32 + 1 is not bit 1
    ([7, 7], [0, 0], [M64, 2], None, 0, [(0, M64, 2, 1, 2)]),                        # the sum wraps
    ([7, 7], [4, 5], [0, 0], None, 0, [(4, 0, 0, 0, 2)]),                            # all zero: the first entry's key
])
def test_row_top_by_hand(first, second, values, chosen, bits, want):
    words = None if chosen is None else rt.bitmap(chosen, bits)
    got = rt.row_top(_u64(first), _u64(second), _u64(values), words, bits)
    assert list(zip(*[g.tolist() for g in got])) == want


@pytest.mark.parametrize("top,nxt,total,rule,want", [
    (0, 0, 0, (0, 0, 1), rt.ROW_NONE),                           # min_value 0 still wants a top of 1
    (4, 0, 4, (5, 0, 1), rt.ROW_NONE),
    (5, 5, 10, (1, 0, 1), rt.ROW_MIXED),                         # a tied top is never assigned
    (5, 4, 9, (1, 0, 1), rt.ROW_ASSIGNED),                       # no share test
    (6, 3, 9, (1, 2, 3), rt.ROW_ASSIGNED),                       # 6 * 3 == 2 * 9: equality passes
    (6, 4, 10, (1, 2, 3), rt.ROW_MIXED),                         # 18 < 20
    (1 << 63, 1, (1 << 63) + 1, (1, 3, 3), rt.ROW_MIXED),        # 3 * 2^63 < 3 * (2^63 + 1): needs more than 64 bits
    (1 << 63, 0, 1 << 63, (1, 3, 3), rt.ROW_ASSIGNED),
])
def test_assign_by_hand(top, nxt, total, rule, want):
    cls, counts = rt.assign(_u64([top]), _u64([nxt]), _u64([total]), *rule)
    assert cls.tolist() == [want] and counts["rows"] == 1 and counts["assigned"] + counts["none"] + counts["mixed"] == 1


# ---- the layers --------------------------------------------------------------------------------------------------------
def test_the_library_exports_both_entry_points_with_the_header_s_argument_counts():
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    import ibu_amd
    for name, argc in NAMES.items():
        assert hasattr(so, name), name
        assert hasattr(ibu_amd.lib, name) and len(_lib.SIGNATURES[name][1]) == argc
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == argc, name
    for method in ("matrix_row_top", "assign_rows", "assign_features"):
        assert callable(getattr(ibu_amd.Context, method))
    assert (ibu_amd.NO_KEY, ibu_amd.ROW_ASSIGNED, ibu_amd.ROW_NONE, ibu_amd.ROW_MIXED) == (rt.NO_KEY, rt.ROW_ASSIGNED, rt.ROW_NONE, rt.ROW_MIXED)
    for p in ("include/ibu.hpp", "bindings/rust/src/ffi.rs", "bindings/rust/src/lib.rs"):
        text = open(os.path.join(ROOT, *p.split("/"))).read()
        assert all(name in text for name in NAMES), p


def test_ctypes_structs_have_the_sizes_the_header_compiles_to(tmp_path):
    from ibu_amd import _lib
    twins = {"ibu_assign_rule_t": _lib.CAssignRule, "ibu_assign_counts_t": _lib.CAssignCounts}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ibu_hip.h"\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n in twins)
                   + '  printf("no_key %d\\n", IBU_NO_KEY == 0xFFFFFFFFFFFFFFFFull);\n'
                   + '  printf("classes %d\\n", IBU_ROW_ASSIGNED * 100 + IBU_ROW_NONE * 10 + IBU_ROW_MIXED);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got.pop("no_key") == "1" and got.pop("classes") == "12"
    assert {n: int(v) for n, v in got.items()} == {n: C.sizeof(t) for n, t in twins.items()} == {"ibu_assign_rule_t": 24, "ibu_assign_counts_t": 32}


def test_kernels_are_in_the_library_and_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = kernel_resources.all_kernels(_lib.SO_PATH)
    mine = {k: v for k, v in ks.items() if k.startswith("ibu_k_rowtop_")}
    assert sorted(mine) == ["ibu_k_rowtop_assign", "ibu_k_rowtop_finish", "ibu_k_rowtop_reduce"]
    assert all(v.get("private_segment_fixed_size", 0) == 0 and not v.get("uses_dynamic_stack", 0) for v in mine.values()), mine
    # no LDS: the scan runs on lane shuffles; the assign has the workgroup totals of block_accumulate, three u64 per wave, and no more
    assert {k: v.get("group_segment_fixed_size", 0) for k, v in mine.items()} == {
        "ibu_k_rowtop_assign": 4 * 3 * 8, "ibu_k_rowtop_finish": 0, "ibu_k_rowtop_reduce": 0}, mine


def test_count_file_names_the_assign_option(tmp_path):
    text = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    usage = text[text.index('"usage: count_file'):]
    usage = usage[:usage.index("return 2;")]
    assert "--assign=min:A[,share:NUM/DEN]" in usage
