"""ibu_partition_records without a GPU: the numpy statement against a plain loop, the plan's arithmetic (compiled from
ibu_amd/csrc/partition_plan.hpp into a small program), the kernels in the code object, the binding, and the demux_file example's
refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import partition_np as pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibu_amd", "csrc")
PLAN_NS = [0, 1, 2047, 2048, 2049, 10**9, 2**40 - 1]
PLAN_PARTS = [1, 2, 64, 65, 255]


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def _maps(n_parts):
    rng = np.random.default_rng(n_parts)
    many_to_one = (np.arange(256) % n_parts).astype(np.uint8)    # non-injective: every class goes somewhere
    holes = many_to_one.copy()
    holes[rng.random(256) < 0.4] = pnp.NONE
    holes[255] = n_parts - 1                                     # class 255 itself is kept
    return [None, many_to_one, holes, np.full(256, pnp.NONE, np.uint8)]


@pytest.mark.parametrize("n_parts", [1, 2, 3, 7, 64, 255])
def test_numpy_statement_agrees_with_a_loop(n_parts):
    rng = np.random.default_rng(100 + n_parts)
    for n in (0, 1, 2, 65, 500):
        recs = np.arange(n, dtype=np.uint64)                     # the input position stands for the record
        for lo, hi in ((0, 256), (0, max(n_parts // 2, 1)), (250, 256)):
            cls = rng.integers(lo, hi, n).astype(np.uint8)
            for m in _maps(n_parts):
                got, off, order = pnp.partition(recs, cls, m, n_parts)
                want_order, want_off = pnp.partition_loop(cls, m, n_parts)
                assert order.tolist() == want_order and off.tolist() == want_off and got.tolist() == want_order
                assert off.dtype == np.uint64 and len(off) == n_parts + 1 and off[-1] == len(order)


def test_map_rules():
    assert pnp.check_map(pnp.identity(1), 1) and pnp.check_map(pnp.identity(255), 255)
    assert not pnp.check_map(pnp.identity(4), 0) and not pnp.check_map(pnp.identity(4), 256)
    m = pnp.identity(4)
    m[9] = 4
    assert not pnp.check_map(m, 4) and pnp.check_map(m, 5)
    assert (pnp.identity(255)[:255] == np.arange(255)).all() and pnp.identity(255)[255] == pnp.NONE


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
PLAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "partition_plan.hpp"
int main(int argc, char** argv) {
  printf("const %llu %llu %u\n", (unsigned long long)ibu::kPartitionScratchConst, (unsigned long long)ibu::kPartitionMaxEntries, ibu::kPartitionMinUnit);
  for (int i = 1; i + 1 < argc; i += 2) {
    const unsigned long long n = strtoull(argv[i], 0, 10);
    const unsigned parts = (unsigned)strtoul(argv[i + 1], 0, 10);
    const ibu::PartitionPlan p = ibu::partition_plan(n, parts);
    printf("%llu %u %u %llu %llu %llu %d\n", n, parts, p.unit, (unsigned long long)p.nunits, (unsigned long long)p.entries,
           (unsigned long long)p.scratch_bytes, p.ok ? 1 : 0);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "plan.cpp").write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(d / "plan.cpp"), "-o", str(d / "plan")])

    def run(pairs):
        out = subprocess.run([str(d / "plan")] + [str(v) for p in pairs for v in p], capture_output=True, text=True, check=True).stdout.splitlines()
        const = [int(v) for v in out[0].split()[1:]]
        return const, [tuple(int(v) for v in ln.split()) for ln in out[1:]]
    return run


def test_plan(plan):
    (const, max_entries, min_unit), rows = plan([(n, p) for n in PLAN_NS for p in PLAN_PARTS])
    assert min_unit == 2048 and max_entries < 2**32 and const <= 4096
    assert len(rows) == len(PLAN_NS) * len(PLAN_PARTS)
    refused = 0
    for n, parts, unit, nunits, entries, scratch, ok in rows:
        assert unit >= 2048 and unit & (unit - 1) == 0 and unit >= 64 * parts and (unit == 2048 or unit < 128 * parts), (n, parts, unit)
        assert nunits * unit >= n and (nunits == 0 or (nunits - 1) * unit < n)
        assert entries == parts * nunits
        assert scratch == 8 * (1 + entries + parts + 1)
        assert scratch <= n // 8 + const, (n, parts, scratch)
        assert ok == (entries <= max_entries)
        refused += not ok
    by_key = {(r[0], r[1]): r for r in rows}
    assert by_key[(2**40 - 1, 255)][6] == 0 and by_key[(2**40 - 1, 65)][6] == 0, "an over-long table is refused"
    assert by_key[(10**9, 255)][6] == 1 and by_key[(2**40 - 1, 1)][6] == 1 and refused >= 2


def test_plan_refuses_part_counts_out_of_range(plan):
    _, rows = plan([(1000, 0), (1000, 256), (1000, 255)])
    assert [r[6] for r in rows] == [0, 0, 1]


def test_units_match_what_the_gpu_test_mirrors(plan):
    _, rows = plan([(1, p) for p in range(1, 256)])
    assert [r[2] for r in rows] == [pnp.unit_of(p) for p in range(1, 256)]
    src = open(os.path.join(CSRC, "kcommon.hpp")).read()
    m = re.search(r"kScanBlock = (\d+), kScanPer = (\d+);", src)
    from tests.test_gpu_partition import SCAN_STEP, U
    assert int(m.group(1)) * int(m.group(2)) == SCAN_STEP == 16384 and U == pnp.unit_of(255) == 16384


# ---- the code object and the binding ----------------------------------------------------------------------------------------------
def test_kernels_are_in_the_code_object():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from ibu_amd import _lib
    ks = kernel_resources.all_kernels(_lib.SO_PATH)
    for name in ("ibu_k_partition_count", "ibu_k_partition_scan", "ibu_k_partition_scatter"):
        assert name in ks, name
        k = ks[name]
        assert k["private_segment_fixed_size"] == 0 and not k.get("uses_dynamic_stack", 0), (name, k)
        assert 0 < k["group_segment_fixed_size"] <= 65536, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
    assert "ibu_k_select_scan" in ks and "ibu_k_select_count" in ks and "ibu_k_select_scatter" in ks
    assert any("ibu_k_sort_scatter" in k for k in ks) and any("ibu_k_sort_elem_scatter" in k or "ibu_k_sort_compress<true, 3, false>" in k for k in ks)


def test_symbol_is_exported_and_refuses_a_null_context():
    import ibu_amd
    from ibu_amd import _lib
    lib = C.CDLL(_lib.SO_PATH)
    assert hasattr(lib, "ibu_partition_records") and "ibu_partition_records" in _lib.SIGNATURES
    assert ibu_amd.PART_NONE == 255
    off = (C.c_uint64 * 3)(7, 7, 7)
    rc = ibu_amd.lib.ibu_partition_records(None, None, None, 0, None, 2, None, 0, off, None)
    assert rc != 0 and ibu_amd.lib.ibu_status_name(rc) == b"InvalidArg" and list(off) == [7, 7, 7]
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    assert "#define IBU_PART_NONE 255u" in header


def test_python_layer_without_a_device():
    import ibu_amd
    if ibu_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Context(0).partition_records(0, 0, 0, n_parts=2)
    assert ei.value.kind == "NoDevice"


def test_python_argument_checks_come_before_any_device_call():
    """partition_by_label refuses duplicate labels, none and more than 255 on the host; partition_records needs a map or a part
    count.  A context that was never opened shows that nothing else is looked at."""
    import ibu_amd
    c = ibu_amd.Context.__new__(ibu_amd.Context)
    for bad in ([], [3, 4, 3], list(range(256)), [0, 256], [-1]):
        with pytest.raises(ValueError):
            c.partition_by_label(None, None, 10, bad)
    with pytest.raises(ValueError):
        c.partition_records(None, None, 10)
    with pytest.raises(ValueError):
        c.partition_records(None, None, 10, part_of=np.zeros(255, np.uint8))


# ---- the example ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def demux(tmp_path_factory):
    from ibu_amd import _lib
    exe = tmp_path_factory.mktemp("demux") / "demux_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "demux_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    return str(exe)


def _input(tmp_path, bc_len=16):
    import ibu_amd
    recs = ibu_amd.records_array([(1, 2, 3), (4, 5, 6), (7, 8, 9)])
    wr = ibu_amd.Writer.from_path(str(tmp_path / "in.ibu"), ibu_amd.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    return str(tmp_path / "in.ibu")


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_demux_file_usage(demux, tmp_path):
    src = _input(tmp_path)
    (tmp_path / "l.txt").write_text("ACGTACGTACGTACGT 1\n")
    for args in ((), (src,), (src, str(tmp_path / "l.txt")), (src, str(tmp_path / "l.txt"), str(tmp_path / "o"), "extra"),
                 ("--nonsense", src, str(tmp_path / "l.txt"), str(tmp_path / "o")), ("--missing", src, str(tmp_path / "l.txt"))):
        r = _run(demux, *args)
        assert r.returncode == 2 and "usage: demux_file [--missing] IN LABELS.txt OUT_PREFIX" in r.stderr, args
    assert sorted(os.listdir(tmp_path)) == ["in.ibu", "l.txt"]


def test_demux_file_refuses_bad_files_before_the_device(demux, tmp_path):
    src = _input(tmp_path)
    good = tmp_path / "good.txt"
    good.write_text("ACGTACGTACGTACGT 1\nTTTTACGTACGTACGT 200\n")
    (tmp_path / "short.ibu").write_bytes(b"junk")
    (tmp_path / "magic.ibu").write_bytes(b"\0" * 64)
    cases = [
        (str(tmp_path / "none.ibu"), str(good), None),
        (str(tmp_path / "short.ibu"), str(good), None),
        (str(tmp_path / "magic.ibu"), str(good), None),
        (src, str(tmp_path / "none.txt"), "cannot open"),
        (src, "ACGTACGTACGTACGT 256\n", "label 0 .. 255"),
        (src, "ACGTACGTACGT 1\n", "16-base barcode"),
        (src, "ACGTACGTACGTACGT\n", "16-base barcode"),
        (src, "ACGTACGTACGTACGN 1\n", "outside ACGT"),
        (src, "\n\n", "empty"),
        (src, "".join(f"{''.join('ACGT'[(k >> (2 * i)) & 3] for i in range(16))} {k}\n" for k in range(256)), "256 distinct labels"),
    ]
    for k, (inp, labels, text) in enumerate(cases):
        if "\n" in labels:
            (tmp_path / f"l{k}.txt").write_text(labels)
            labels = str(tmp_path / f"l{k}.txt")
        r = _run(demux, "--missing", inp, labels, str(tmp_path / "out"))
        assert r.returncode == 1 and r.stderr.startswith("error: "), (k, r.returncode, r.stderr)
        assert "device" not in r.stderr.lower() and "hip" not in r.stderr.lower(), (k, r.stderr)
        assert text is None or text in r.stderr, (k, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]


def test_demux_file_creates_no_file_when_a_device_call_is_refused(demux, tmp_path):
    import ibu_amd
    if ibu_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    src = _input(tmp_path)
    (tmp_path / "l.txt").write_text("ACGTACGTACGTACGT 1\n")
    r = _run(demux, src, str(tmp_path / "l.txt"), str(tmp_path / "out"))
    assert r.returncode == 1 and "NoDevice" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.ibu", "l.txt"]
