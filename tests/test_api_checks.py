"""The argument checks the entry points of the C ABI share (ibu_amd/csrc/api_checks.hpp), driven on the host through
tests/cpp/test_api_checks.cpp: the overlap test at its edges, the pointer and 2^40 checks, and for every helper that sets an error
its status, detail words and exact message as ibu_last_error reports them.  The expected messages are the ABI's, written out here.
Runs without a GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/test_api_checks"])
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "test_api_checks")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    by_name = {x["case"]: x for x in lines}
    assert len(by_name) == len(lines)
    return by_name


@pytest.mark.parametrize("name,want", [
    ("disjoint", False),
    ("adjacent", False),                  # end == begin shares no byte
    ("one_shared_byte", True),
    ("inside", True),
    ("identical", True),
    ("first_empty", False),               # an empty range inside the other
    ("both_empty", False),
    ("ends_at_top_disjoint", False),      # a + a_bytes would wrap to 0
    ("ends_at_top_adjacent", False),
    ("ends_at_top_shared", True),
    ("huge_length_from_low", True),
])
def test_ranges_overlap(cases, name, want):
    assert cases[name]["overlap"] is want and cases[name]["swapped"] is want


def _refused(case, a, b, message):
    assert case["status"] == "InvalidArg" and case["code"] == case["rc"] != 0
    assert (case["a"], case["b"]) == (a, b)
    assert case["message"] == message


def test_u64_pointer_checks(cases):
    assert cases["aligned8"]["values"] == [1, 1, 0, 0]
    for ok in ("ptr_mod8_0", "ptrs_both_good"):
        assert cases[ok] == {"case": ok, "rc": 0}
    _refused(cases["ptr_null"], 0, 0, "Invalid argument: d_records must be non-NULL and 8-byte aligned")
    _refused(cases["ptr_mod8_1"], 0, 0, "Invalid argument: d_sorted_records must be non-NULL and 8-byte aligned")
    _refused(cases["ptr_mod8_4"], 0, 0, "Invalid argument: d_codes must be non-NULL and 8-byte aligned")
    _refused(cases["ptrs_second_null"], 0, 0, "Invalid argument: d_records / d_tmp must be non-NULL and 8-byte aligned")
    _refused(cases["ptrs_second_mod8_4"], 0, 0, "Invalid argument: d_a / d_b must be non-NULL and 8-byte aligned")


def test_the_2_40_limit(cases):
    assert cases["limit_just_below"] == {"case": "limit_just_below", "rc": 0}
    _refused(cases["limit_at"], 0, 0, "Invalid argument: sort_records handles fewer than 2^40 records per call")
    _refused(cases["limit_size_max"], 0, 0, "Invalid argument: subsample_class handles fewer than 2^40 rows per call")
    _refused(cases["limit_values"], 0, 0, "Invalid argument: rank_select handles fewer than 2^40 values per call")
    _refused(cases["limit_codes"], 0, 0, "Invalid argument: abundance_counts handles fewer than 2^40 codes per call")


def test_capacity_errors_carry_need_and_capacity(cases):
    _refused(cases["capacity_pairs"], 12, 11, "Invalid argument: output capacity 11 is smaller than the 12 entries (see *n_pairs)")
    _refused(cases["capacity_select"], 64, 63, "Invalid argument: output capacity 63 is smaller than the 64 records kept (see *n_out)")
    _refused(cases["capacity_metrics"], 1 << 33, 7, "Invalid argument: output capacity 7 is smaller than the 8589934592 barcodes (see *n_barcodes)")
