"""tools/aggbench.py --mtx checks the library against the entry table it laid: replayed here on the CPU, the numpy statement
(tests/mtx_np.py) finds in that table exactly the rows, the row pointers and the largest printed values the tool's layout says, and
the copy the tool compares the body with moves as many bytes as the body does.  The host loop it times compiles and prints what
examples/count_file.cpp prints."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mtx_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def aggbench():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import aggbench
    return aggbench


@pytest.mark.parametrize("n", [1999, 2000, 3 * 1999, 50_001])
def test_mtx_plan_lays_the_rows_it_checks(aggbench, n):
    import torch
    bc, idx, umis, reads = (x.numpy().astype(np.uint64) for x in aggbench.mtx_fill(torch, torch.arange(n, dtype=torch.int64)))
    rows, nf = aggbench.mtx_layout(n)
    ordinals, keys, ptr = mtx_np.matrix_rows(bc)
    assert len(keys) == rows and ptr.tolist() == [min(r * aggbench.MTX_ROW, n) for r in range(rows + 1)]
    assert int(bc.max()) < 1 << (2 * aggbench.MTX_BC_LEN) and int(umis.min()) >= 1 and (reads == 3 * umis + 1).all()
    text, maxima = mtx_np.body(idx.tolist(), ordinals.tolist(), umis.tolist(), 1, 1)
    assert maxima == (nf, rows, int(umis.max())) and text.startswith(b"1 1 %d\n" % int(umis[0])) and text.count(b"\n") == n
    total, copy_bytes = aggbench.mtx_traffic(n, len(text))
    assert total == 48 * n + len(text) and 2 * copy_bytes in (total, total - 1)


def test_mtx_host_loop_prints_what_count_file_prints(tmp_path):
    so = tmp_path / "mtx_host_loop.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tools", "mtx_host_loop.cpp"),
                           "-o", str(so)])
    loop = C.CDLL(str(so)).mtx_host_loop
    loop.restype, loop.argtypes = C.c_double, [C.c_void_p] * 4 + [C.c_size_t, C.c_uint32, C.c_char_p]
    cols = [np.array(v, np.uint64) for v in ([0b11100100, 0], [7, (1 << 64) - 1], [3, 1], [9, 2])]
    out = tmp_path / "lines.txt"
    assert loop(*[c.ctypes.data for c in cols], 2, 4, str(out).encode()) >= 0
    assert out.read_text() == "ACGT\t7\t3\t9\nAAAA\t18446744073709551615\t1\t2\n"
    assert loop(*[c.ctypes.data for c in cols], 2, 4, str(tmp_path / "no" / "such").encode()) == -1
    src = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    assert '"%s\\t%llu\\t%llu\\t%llu\\n", decode(e.first, h.bc_len).c_str()' in src   # the loop the tool stands in for
