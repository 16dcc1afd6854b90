"""One index per molecule (ibu_classify_molecules) — what can be checked without a GPU: the numpy statement of the semantics
(tests/molecule_np.py) against a brute force over the runs and against cases a reader can check by eye, the fixture the GPU
tests use, the entry point in every layer of the ABI, the loud failure on a box without a device, and the example program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import molecule_np as mnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibu_classify_molecules"


@pytest.mark.parametrize("n", [129, 2561, 8193])
@pytest.mark.parametrize("tie_first", [False, True])
def test_numpy_statement_equals_brute_force(n, tie_first):
    recs = mnp.make_sorted(mnp.SEED + n, n)
    cls, tot = mnp.classify(recs, tie_first)
    bcls, btot = mnp.brute_force(recs, tie_first)
    assert cls.dtype == np.uint8 and cls.tobytes() == bcls.tobytes()
    assert tot == btot
    assert tot["reads_kept"] + tot["reads_minor"] + tot["reads_tied"] == n == len(cls)
    assert tot["tied"] > 0 and (tie_first or tot["reads_tied"] > 0)
    assert not tie_first or tot["reads_tied"] == 0, "class 2 never occurs under the flag"
    # the same on the runs of unsorted input
    shuffled = recs[np.random.default_rng(n).permutation(n)]
    cls, tot = mnp.classify(shuffled, tie_first)
    bcls, btot = mnp.brute_force(shuffled, tie_first)
    assert cls.tobytes() == bcls.tobytes() and tot == btot and tot["molecules"] > mnp.classify(recs)[1]["molecules"]


@pytest.mark.parametrize("n", [63, 129, 2561, 8193, 100_003])
def test_the_fixture_has_what_it_claims(n):
    recs = mnp.make_sorted(mnp.SEED + n, n)
    cls, tot = mnp.classify(recs)
    share = [float((cls == c).mean()) for c in (0, 1, 2)]
    print(n, "kept / minor / tied shares", share, tot)
    assert all(s > 0.03 for s in share), "all three classes"
    mols = mnp.molecule_runs(recs)
    reads = [[r for _, r in m] for m in mols]
    winner_not_first = sum(1 for r in reads if len(r) >= 2 and r.count(max(r)) == 1 and r[0] != max(r))
    winner_last = sum(1 for r in reads if len(r) >= 2 and r.count(max(r)) == 1 and r[-1] == max(r))
    assert winner_not_first > 0 and winner_last > 0
    if n >= 2561:
        assert any(len(r) == 3 and r[0] == r[1] == r[2] for r in reads), "a three-way tie"
    if n >= 8193:
        k = next(j for j, r in enumerate(reads) if sorted(r) == [1, 3, 3])
        first = sum(sum(r) for r in reads[:k])
        assert cls[first:first + 7].tolist() == [2] * 7, "a (3, 3, 1) molecule is tied: all seven records are class 2"


def _classes(rows, tie_first=False):
    cls, tot = mnp.classify(mnp.recs_of(rows), tie_first)
    bcls, btot = mnp.brute_force(mnp.recs_of(rows), tie_first)
    assert cls.tolist() == bcls.tolist() and tot == btot
    assert tot["reads_kept"] + tot["reads_minor"] + tot["reads_tied"] == len(rows)
    return cls.tolist(), tot


def test_hand_written_cases():
    cls, tot = _classes([])
    assert cls == [] and all(v == 0 for v in tot.values())
    cls, tot = _classes([(7, 8, 9)])
    assert cls == [0] and (tot["molecules"], tot["candidates"], tot["resolved"], tot["tied"], tot["reads_kept"]) == (1, 1, 0, 0, 1)
    for flag in (False, True):
        cls, tot = _classes([(1, 1, 5), (1, 1, 5), (1, 1, 6)], flag)            # reads (2, 1)
        assert cls == [0, 0, 1] and (tot["resolved"], tot["tied"]) == (1, 0)
        cls, tot = _classes([(1, 1, 5), (1, 1, 6), (1, 1, 6)], flag)            # reads (1, 2): the winner is the last candidate
        assert cls == [1, 0, 0] and (tot["resolved"], tot["tied"], tot["reads_minor"]) == (1, 0, 1)
    cls, tot = _classes([(1, 1, 5), (1, 1, 6)])                                # reads (1, 1)
    assert cls == [2, 2] and (tot["resolved"], tot["tied"], tot["reads_tied"]) == (0, 1, 2)
    cls, tot = _classes([(1, 1, 5), (1, 1, 6)], True)
    assert cls == [0, 1] and (tot["resolved"], tot["tied"], tot["reads_tied"]) == (0, 1, 0), "tied is counted under the flag too"
    cls, tot = _classes([(1, 1, 5)] * 2 + [(1, 1, 6)] * 2 + [(1, 1, 7)])       # reads (2, 2, 1): the smaller candidate is tied too
    assert cls == [2] * 5 and tot["tied"] == 1
    cls, tot = _classes([(1, 1, 5)] * 2 + [(1, 1, 6)] * 2 + [(1, 1, 7)], True)
    assert cls == [0, 0, 1, 1, 1]
    cls, tot = _classes([(1, 1, 4)] + [(1, 1, 5)] * 2 + [(1, 1, 6)] * 2, True)  # reads (1, 2, 2): the first AT BEST, not the first
    assert cls == [1, 0, 0, 1, 1]
    # an interrupted molecule on unsorted input is two molecules: (1,1) has reads (2) and then (1, 1)
    cls, tot = _classes([(1, 1, 5), (1, 1, 5), (2, 1, 5), (1, 1, 5), (1, 1, 6)])
    assert cls == [0, 0, 0, 2, 2] and (tot["molecules"], tot["candidates"], tot["tied"]) == (3, 4, 1)
    # an index that returns inside a molecule is a new candidate: reads (1, 1, 1)
    cls, tot = _classes([(1, 1, 5), (1, 1, 6), (1, 1, 5)])
    assert cls == [2, 2, 2] and tot["candidates"] == 3
    hi = 1 << 63
    cls, tot = _classes([(hi, hi, hi), (hi, hi, hi), (hi, hi, hi + 1), (hi, hi + 1, hi + 1), (hi + 1, hi + 1, hi + 1)])
    assert cls == [0, 0, 1, 0, 0] and (tot["molecules"], tot["candidates"], tot["resolved"]) == (3, 4, 1)
    # the matrix of the resolved molecules: barcode 10 / umi 7 was seen with index 0 twice and index 1 once
    recs = mnp.recs_of([(10, 7, 0), (10, 7, 0), (10, 7, 1), (10, 8, 1), (20, 5, 0), (20, 5, 1)])
    assert mnp.resolved_matrix(recs) == {(10, 0): [2, 1], (10, 1): [1, 1]}
    assert mnp.resolved_matrix(recs, True) == {(10, 0): [2, 1], (10, 1): [1, 1], (20, 0): [1, 1]}


def test_entry_point_exists_in_every_layer():
    from ibu_amd import _lib
    header = open(os.path.join(ROOT, "include", "ibu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    so = C.CDLL(_lib.SO_PATH)
    assert re.search(r"\b%s\s*\(" % NAME, code), "not declared in ibu_hip.h"
    assert hasattr(so, NAME), "not exported"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 7
    assert re.search(r"pub fn %s\s*\(" % NAME, ffi) and "pub struct ibu_molecule_counts_t" in ffi
    assert C.sizeof(_lib.CMoleculeCounts) == 64
    for name, value in (("IBU_MOLECULE_KEPT", "0"), ("IBU_MOLECULE_MINOR", "1"), ("IBU_MOLECULE_TIED", "2"), ("IBU_MOLECULES_TIE_FIRST", "1u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    import ibu_amd
    assert (ibu_amd.MOLECULE_KEPT, ibu_amd.MOLECULE_MINOR, ibu_amd.MOLECULE_TIED, ibu_amd.MOLECULES_TIE_FIRST) == (0, 1, 2, 1)
    assert hasattr(ibu_amd.Context, "classify_molecules")
    assert ibu_amd.MoleculeCounts._fields == mnp.TOTALS
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ibu.hpp")).read()
    assert re.search(r"pub fn classify_molecules\s*\(", lib_rs)
    assert re.search(r"\bclassify_molecules\s*\(", hpp)
    so.ibu_abi_revision.restype = C.c_uint32
    assert so.ibu_abi_revision() == 6, "a new entry point changes no signature"


def test_kernels_are_in_the_code_object():
    from ibu_amd import _lib
    out = subprocess.run(["strings", "-a", _lib.SO_PATH], capture_output=True, text=True).stdout
    for k in ("ibu_k_molecules_emit", "ibu_k_molecules_verdict", "ibu_k_molecules_chains", "ibu_k_molecules_fix", "ibu_k_class_fill"):
        assert k in out, k
    for k in ("ibu_k_molecules_fill", "ibu_k_cells_fill"):   # one class fill (k_aggregate.hip) serves both
        assert k not in out, k


def test_classify_molecules_fails_loudly_without_gpu():
    """No device: NoDevice from the library — there is no host form to fall back to."""
    import ibu_amd
    from ibu_amd import _lib
    so = C.CDLL(_lib.SO_PATH)
    c = _lib.CMoleculeCounts()
    assert so.ibu_classify_molecules(None, None, C.c_size_t(1), 0, None, C.byref(c), None) != 0, "a NULL context is an error, never a host computation"
    assert so.ibu_classify_molecules(None, None, C.c_size_t(0), 0, None, None, None) != 0
    if ibu_amd.device_count() > 0:
        return
    with pytest.raises(ibu_amd.IbuError) as ei:
        ibu_amd.Context(0).classify_molecules(None, 1)
    assert ei.value.kind == "NoDevice"


def test_count_file_example_compiles_with_the_resolve_option(tmp_path):
    from ibu_amd import _lib
    src = open(os.path.join(ROOT, "examples", "count_file.cpp")).read()
    assert "--resolve=first" in src and "classify_molecules" in src
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "count_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    for args in ([], ["--resolve"], ["--resolve=first"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.returncode == 2 and "usage: count_file" in r.stderr


def test_candidate_layouts_of_the_block_seam_tests():
    """tests/test_gpu_block_seams.py lays molecules at the boundaries of the 1024-candidate verdict blocks: the builder round-trips,
    the numpy statement equals the brute force on every layout at the largest size, and the block sizes the layouts assume are
    still the source's."""
    # lay_candidates -> _runs gives the table back, for sorted records
    reads, heads = [1, 2, 1, 1, 3, 1], [True, False, True, False, False, True]
    recs = mnp.lay_candidates(reads, heads)
    starts, mol = mnp._runs(recs)
    assert starts.tolist() == [0, 1, 3, 4, 5, 8] and mol.tolist() == [0, 0, 1, 1, 1, 2] and len(recs) == 9
    assert recs.tobytes() == mnp.cnp.sort_records(recs).tobytes()
    assert [[r for _, r in m] for m in mnp.molecule_runs(recs)] == [[1, 2], [1, 1, 3], [1]]
    ncand = mnp.BLOCK_SIZES[-1]
    plan = mnp.seam_plan(ncand)
    assert ncand == 1024 * 1031 + 7 and sum(len(a) for a in plan) > 150
    brute_long = 0
    for laid in plan:
        reads, mol_head, pieces = mnp.seam_table(ncand, laid)
        hd = np.flatnonzero(mol_head)
        for (K, spec), p in zip(laid, pieces):
            # the piece with a few molecules on either side, cut at molecule heads: whole molecules, classified as in the whole table
            lo, hi = int(hd[max(np.searchsorted(hd, p["lo"]) - 3, 0)]), int(hd[min(np.searchsorted(hd, p["hi"]) + 3, len(hd) - 1)])
            assert lo < p["lo"] and p["hi"] < hi
            sub = {"head_checks": [(c - lo, h) for c, h in p["head_checks"]], "classes": [(c - lo, x, y) for c, x, y in p["classes"]]}
            recs = mnp.lay_candidates(reads[lo:hi], mol_head[lo:hi])
            want = {f: mnp.classify(recs, f) for f in (False, True)}
            mnp.check_seam_table(reads[lo:hi], mol_head[lo:hi], [sub], recs, want)   # the round trip, and the piece lies where it says
            rows = np.concatenate([[0], np.cumsum(reads[lo:hi])])
            if spec[0] == "long":
                # every candidate of the long molecule, from the rule by eye: the one with two reads is kept and the rest minor;
                # with two of them, or none, all are tied, or the first at best is kept under tie_first
                a, b, twos = p["lo"] - lo, p["hi"] - lo, [t - lo for t in p["twos"]]
                c = np.arange(a, b)
                if len(twos) == 1:
                    plain = first = np.where(c == twos[0], mnp.KEPT, mnp.MINOR)
                else:
                    plain, first = np.full(b - a, mnp.TIED), np.where(c == (twos[0] if twos else a), mnp.KEPT, mnp.MINOR)
                for f, exp in ((False, plain), (True, first)):
                    assert (want[f][0][rows[a]:rows[b]] == np.repeat(exp, reads[lo:hi][a:b])).all(), spec
                if spec[1] != "tie_round_seam":
                    continue
                brute_long += 1
            for f in (False, True):
                assert mnp.brute_force(recs, f)[0].tobytes() == want[f][0].tobytes(), (K, spec, f)
    assert brute_long == 1
    # the seams the layouts sit on are the source's
    src = open(os.path.join(ROOT, "ibu_amd", "csrc", "k_molecules.hip")).read()
    walk = open(os.path.join(ROOT, "ibu_amd", "csrc", "runs_walk.hpp")).read()
    stitch = open(os.path.join(ROOT, "ibu_amd", "csrc", "k_saturation.hip")).read()
    assert re.search(r"kMolItems = 4;", src) and re.search(r"kMolBlock = kSortThreads \* kMolItems;", src) and re.search(r"kSortThreads = 256;", walk)
    assert re.search(r"base \+= kMolBlock\)", src), "the chains scan takes one block of summaries per round"
    body = stitch[stitch.index("ibu_k_saturation_stitch("):stitch.index("ibu_k_saturation_points(")]
    assert "s_base += 4 * kSortThreads" in body and "s_base + 4 * threadIdx.x" in body
    assert mnp.MOL_BLOCK == 256 * 4
