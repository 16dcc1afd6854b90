"""The numpy statement of the per-barcode labels (tests/label_np.py) against a brute-force Python dict, and what the library says
about labels on a host without a device.  Runs without a GPU."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import label_np as lnp
from tests import whitelist_np as wnp

BC_LENS = [1, 5, 16, 32]


def _case(bc_len, ones=None, n=400, seed=0):
    """-> (whitelist, codes set, their labels, barcodes).  ones (32 bases only): True = the all-ones key is an entry, False = it is
    read but is no entry."""
    rng = np.random.default_rng([0x1AB0100, bc_len, seed, int(bool(ones))])
    w = 3 if bc_len == 1 else 40
    wl = lnp.whitelist(rng, bc_len, w, ones=bool(ones))
    codes, labs = lnp.label_pattern(wl, "rank256")
    labs = (labs.astype(np.int64) * 37 % 256).astype(np.uint8)          # 40 entries still reach labels above 7 and above 127
    bc = lnp.barcodes(rng, wl, bc_len, n)
    if bc_len < 32:
        bc[::3] |= np.uint64(1) << np.uint64(2 * bc_len)                 # a bit above 2*bc_len on every third record, entry or not
        bc[5::7] |= np.uint64(1) << np.uint64(63)
    if ones is not None:
        bc[rng.integers(0, n, 20)] = np.uint64(wnp.FREE)
    return wl, codes, labs, bc


@pytest.mark.parametrize("bc_len,ones", [(b, None) for b in BC_LENS] + [(32, True), (32, False)])
def test_statement_matches_a_python_dict(bc_len, ones):
    wl, codes, labs, bc = _case(bc_len, ones)
    lb = lnp.Labels(wl, bc_len, fill=200)
    table = lnp.brute_table(wl, bc_len, fill=200)
    if ones is not None:
        assert (np.uint64(wnp.FREE) in wl) == ones and (bc == np.uint64(wnp.FREE)).any()
    # set: the codes of the pattern, two that are no entries and, below 32 bases, an entry with a bit above 2*bc_len
    out = lnp.outsiders(np.random.default_rng(1), wl, bc_len, 2)
    extra = [out] + ([codes[:1] | np.uint64(1 << (2 * bc_len))] if bc_len < 32 else [])
    all_codes = np.concatenate([codes] + extra)
    all_labs = np.concatenate([labs, np.full(len(all_codes) - len(codes), 9, np.uint8)])
    skipped = lnp.set_labels(lb, all_codes, all_labs)
    assert skipped == lnp.brute_set(table, bc_len, all_codes, all_labs) == len(all_codes) - len(codes)
    assert {int(c): int(v) for c, v in zip(lb.wl, lb.lab)} == table
    assert len(codes) == len(lb.wl) - len(lb.wl) // 5 and int((lb.lab == 200).sum()) >= len(lb.wl) // 5, "fill survives on the entries never set"
    # get: entries, non-entries, codes with a high bit
    probe = np.concatenate([np.unique(wl), all_codes[len(codes):]])
    want = [table[int(c)] if not int(c) >> (2 * bc_len) and int(c) in table else 77 for c in probe]
    assert lnp.get_labels(lb, probe, missing=77).tolist() == want
    # label_records, plain and match mode
    for missing_class in (255, 3):
        cls, hist = lnp.label_records(lb, bc, missing_class=missing_class)
        bcls, bhist = lnp.brute_label(table, bc_len, bc, missing_class=missing_class)
        assert (cls == bcls).all() and (hist == bhist).all()
        assert int(hist.sum()) == len(bc) and hist[256] > 0
    for match in (0, 7, 200, int(labs[0])):
        cls, hist = lnp.label_records(lb, bc, match=match)
        bcls, bhist = lnp.brute_label(table, bc_len, bc, match=match)
        assert (cls == bcls).all() and (hist == bhist).all() and int(hist.sum()) == len(bc)


@pytest.mark.parametrize("bc_len", BC_LENS)
def test_match_mode_is_plain_mode_mapped(bc_len):
    wl, codes, labs, bc = _case(bc_len, seed=1)
    lb = lnp.Labels(wl, bc_len, fill=0)
    lnp.set_labels(lb, codes, labs)
    plain, hist = lnp.label_records(lb, bc, missing_class=255)
    found = np.isin(bc & wnp.mask(bc_len) if bc_len < 32 else bc, wl)
    assert int(hist[256]) == int((~found).sum())
    for match in sorted({0, 7, 200, 255, int(labs[1])}):
        cls, hist_m = lnp.label_records(lb, bc, match=match)
        want = np.where(~found, lnp.MISSING, np.where(plain == match, lnp.IS, lnp.OTHER))
        assert (cls == want).all() and (hist_m == hist).all()
        assert int((cls == lnp.IS).sum()) == int(hist[match])


def test_upper_bits_are_ignored_and_never_an_entry():
    bc_len = 5
    wl, codes, labs, bc = _case(bc_len, seed=2)
    lb = lnp.Labels(wl, bc_len)
    lnp.set_labels(lb, codes, labs)
    low = bc & wnp.mask(bc_len)
    assert (low != bc).any()
    a, b = lnp.label_records(lb, bc), lnp.label_records(lb, low)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    high = codes | np.uint64(1 << (2 * bc_len))
    assert lnp.set_labels(lb, high, labs) == len(high) and (lnp.get_labels(lb, high, 9) == 9).all()


def test_fails_loudly_without_gpu():
    """No device: NoDevice from the library — there is no host form of the labels to fall back to."""
    import ibu_amd
    if ibu_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Labels(None, None)
    assert ei.value.kind == "NoDevice"
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Context.label_records(types.SimpleNamespace(_c=None), None, None, 10, hist=True)
    assert ei.value.kind == "NoDevice"
    so = ibu_amd.lib
    h = C.c_void_p()
    rc = so.ibu_labels_create(None, None, 255, None, C.byref(h))
    assert so.ibu_status_name(rc) == b"NoDevice" and not h.value
    hist = (C.c_uint64 * 257)(*([9] * 257))
    rc = so.ibu_label_records(None, None, None, 10, 0, 0, 255, None, hist, None)
    assert so.ibu_status_name(rc) == b"NoDevice" and list(hist) == [9] * 257


def test_python_layer_refuses_what_a_byte_cannot_hold():
    import ibu_amd
    fake = types.SimpleNamespace(_c=None)
    top = types.SimpleNamespace(n_rows=1)
    with pytest.raises(ValueError, match="253"):
        ibu_amd.Context.labels_from_assignment(fake, None, top, None, list(range(254)), 16)
    with pytest.raises(ValueError, match="distinct"):
        ibu_amd.Context.labels_from_assignment(fake, None, top, None, [1, 1], 16)
    with pytest.raises(ValueError, match="mixed"):
        ibu_amd.Context.labels_from_assignment(fake, None, top, None, list(range(20)), 16, mixed=19)


def test_every_layer_names_the_new_entry_points():
    import os
    import re
    from ibu_amd import _lib
    import ibu_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = {"ibu_labels_create": 5, "ibu_labels_info": 2, "ibu_labels_destroy": 1, "ibu_labels_set": 7, "ibu_labels_get": 7, "ibu_label_records": 10}
    so = C.CDLL(_lib.SO_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ibu_hip.h")).read(), flags=re.S)
    for name, argc in names.items():
        assert hasattr(so, name) and len(_lib.SIGNATURES[name][1]) == argc, name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == argc, name
    for p in ("include/ibu.hpp", "bindings/rust/src/ffi.rs", "bindings/rust/src/lib.rs"):
        text = open(os.path.join(root, *p.split("/"))).read()
        assert all(name in text for name in names), p
    for method in ("label_records", "labels_from_assignment"):
        assert callable(getattr(ibu_amd.Context, method))
    assert callable(ibu_amd.Whitelist.labels) and (ibu_amd.LABEL_MATCH, ibu_amd.LABEL_IS, ibu_amd.LABEL_OTHER, ibu_amd.LABEL_MISSING) == (1, lnp.IS, lnp.OTHER, lnp.MISSING)
    assert ibu_amd.LABEL_BINS == lnp.BINS == 257
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "new entry points change no signature"


def test_count_file_example_compiles_with_the_label_options(tmp_path):
    import os
    import subprocess
    from ibu_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    for args in (["--keep-label=3", "in.ibu"], ["--label-hist", "in.ibu"], ["--labels=f", "--keep-label=256", "in.ibu"], ["--labels=", "in.ibu"]):
        r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage: count_file" in r.stderr and "--labels=FILE" in r.stderr, (args, r.stderr)


def test_the_byte_check_of_the_shared_argument_checks(tmp_path):
    """api_checks.hpp check_byte, driven with plain g++ as tests/cpp/test_api_checks.cpp drives its neighbours: 255 passes, 256 and
    2^32 - 1 are InvalidArg with the value in detail.a and the argument's name in the message."""
    import os
    import subprocess
    from ibu_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "byte.cpp"
    src.write_text('#include <stdio.h>\n#include "api_checks.hpp"\n#include "ibu_hip.h"\n'
                   "int main() {\n"
                   "  if (ibu::check_byte(0, \"fill\") != IBU_OK || ibu::check_byte(255, \"fill\") != IBU_OK) return 1;\n"
                   "  const uint32_t bad[2] = {256u, 0xFFFFFFFFu};\n"
                   "  for (uint32_t v : bad) {\n"
                   "    const int32_t rc = ibu::check_byte(v, \"missing_class\");\n"
                   "    ibu_error_detail_t d;\n"
                   "    ibu_last_error(&d);\n"
                   "    printf(\"%s|%d|%llu|%s\\n\", ibu_status_name(rc), rc == d.code, (unsigned long long)d.a, d.message);\n"
                   "  }\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "byte"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "ibu_amd", "csrc"),
                           "-I", os.path.join(root, "include"), str(src), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    message = "Invalid argument: missing_class must be at most 255 (it stands for one byte)"
    assert r.stdout.splitlines() == [f"InvalidArg|1|256|{message}", f"InvalidArg|1|4294967295|{message}"]


def test_labels_from_assignment_refuses_two_rows_of_one_barcode():
    """Row barcodes that differ only in bits at or above 2*bc_len are one whitelist entry: refused before anything is built."""
    import ibu_amd

    def column(a):
        return types.SimpleNamespace(download=lambda dtype, count: np.asarray(a, dtype=dtype)[:count])

    fake = types.SimpleNamespace(_c=None, synchronize=lambda stream=None: None)
    keys = [5, 9, 5 | (1 << 40)]
    top = types.SimpleNamespace(n_rows=3, top_key=column([1, 2, 1]))
    with pytest.raises(ValueError, match="one barcode"):
        ibu_amd.Context.labels_from_assignment(fake, column(keys), top, column([0, 0, 0]), [1, 2], 16)
