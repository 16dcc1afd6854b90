"""The ranges of the pull stream over a BGZF file (ibu_stream_open_path; ibu_amd/csrc/bgzf_plan.hpp: plan_range_records, plan_records),
driven through tests/cpp/test_bgzf_ranges.cpp and checked against ibu_shard_range and the bytes the files were written from.  Runs without
a GPU; the driver is compiled here with its own compiler command."""
import json
import math
import os
import struct
import subprocess
import zlib

import pytest

from tests import deflate_craft as dc
from tests.bgzf import bgzf_compress
from tests.test_bgzf_plan import _check_plans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = struct.pack("<IIIIQ8s", 0x21554249, 2, 16, 12, 0, b"\0" * 8)
REFILL = 49_152                                                     # IBU_DEFAULT_BUFFER_SIZE / 24
SLOTS = [1024, REFILL, 65_536, 4 << 20]                             # ring slots after ring_ensure's rounding to 128 records


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def driver(ia, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bin") / "test_bgzf_ranges")
    csrc, lib = os.path.join(ROOT, "ibu_amd", "csrc"), os.path.join(ROOT, "ibu_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_bgzf_ranges.cpp"), "-o", out, "-L" + lib, "-libu_hip", "-Wl,-rpath," + lib,
                           "-lpthread", "-lz"])
    return out


def _targets(file_bytes, n, refills=range(1, 11)):
    """Range targets (compressed bytes) of so many refills per range at the file's ratio, and one far beyond the file."""
    return [math.ceil(file_bytes * m * REFILL / max(n, 1)) + 1 for m in refills] + [1 << 62]


def _run(driver, path, slots, targets, shards=True):
    args = [driver, str(path), ",".join(map(str, slots)), ",".join(map(str, targets))] + ([] if shards else ["noshards"])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    idx = lines[0]
    shards = [x for x in lines[1:] if "n_shards" in x]
    ranges = [x for x in lines[1:] if "slot" in x]
    assert idx["rc"] or lines[-1] == {"past_end": 13}                 # IBU_ERR_INVALID_ARG
    return idx, shards, ranges


def _check_ranges(idx, cases, comp, plain):
    B = idx["blocks"]
    n = (len(plain) - 32) // 24
    counts = set()
    for c in cases:
        slot, target, r = c["slot"], c["target"], c["range_records"]
        per = n if target >= len(comp) else int(n * target / len(comp))
        lcm = slot * REFILL // math.gcd(slot, REFILL)
        unit = lcm if lcm <= per else REFILL
        want = max(-(-n // unit), 1) * unit if per >= n else max((per + unit // 2) // unit, 1) * unit
        assert r % REFILL == 0 and r % unit == 0 and r == want, c
        rs = c["ranges"]
        assert len(rs) == (n + r - 1) // r
        counts.add(len(rs))
        at = 0
        for k, p in enumerate(rs):                                  # the ranges tile the records in order ...
            assert p["rec_first"] == at and p["num"] == (r if k + 1 < len(rs) else n - at), (slot, target, k)
            at += p["num"]
            lo, hi = p["lo"], p["hi"]
            assert (lo, hi) == (32 + 24 * p["rec_first"], 32 + 24 * (p["rec_first"] + p["num"]))
            dev = range(p["dev_first"], p["dev_end"])
            assert idx["lead"] <= p["dev_first"] <= p["dev_end"] <= len(B)
            assert len(p["edges"]) <= 2 and not set(p["edges"]) & set(dev) and all(e >= idx["lead"] for e in p["edges"])
            for j in dev:                                           # ... no device block straddles a range's ends ...
                assert lo <= B[j][2] and B[j][2] + B[j][3] <= hi
            pieces = [(0, idx["head"])] + [(B[j][2], B[j][2] + B[j][3]) for j in list(p["edges"]) + list(dev)]
            cut = sorted((max(a, lo), min(z, hi)) for a, z in pieces if max(a, lo) < min(z, hi))
            pos = lo                                                # ... and its pieces tile its bytes exactly once
            for a, z in cut:
                assert a == pos, (slot, target, k, cut)
                pos = z
            assert pos == hi
            if len(dev):                                            # only the device blocks' bytes cross the link
                assert (p["cbeg"], p["cend"]) == (B[dev[0]][0], B[dev[-1]][0] + B[dev[-1]][1])
            else:
                assert (p["cbeg"], p["cend"]) == (0, 0)
            assert p["crc"] == zlib.crc32(plain[lo:hi])
        assert at == n
    return counts


@pytest.mark.parametrize("block", [20, 4093, 0xFF00])
@pytest.mark.parametrize("n", [0, 1, REFILL - 1, REFILL + 1, 9 * REFILL + 5])
def test_ranges_tile_the_records_and_keep_the_refill(ia, oracle, driver, tmp_path, block, n):
    if block == 20 and n > REFILL + 1:
        n = 2 * REFILL + 7                                          # (a block of 20 bytes: 1.2 M blocks would take the writer too long)
    plain = HDR + oracle.generate(0x1B00020 + n, 0, n, 16, 12).tobytes()
    for eof in (True, False):
        comp = bgzf_compress(plain, block=block, eof=eof)
        path = tmp_path / "f.gz"
        path.write_bytes(comp)
        idx, shards, ranges = _run(driver, path, SLOTS, _targets(len(comp), n))
        assert idx["rc"] == 0 and idx["file_bytes"] == len(comp)
        _check_plans(ia, idx, shards, comp, plain)                 # plan_shard over plan_records: its old plans
        counts = _check_ranges(idx, ranges, comp, plain)
        assert counts == {0} if n == 0 else 1 in counts and (n <= REFILL or 2 in counts)


def test_targets_give_one_to_nine_ranges(oracle, driver, tmp_path):
    n = 60 * REFILL + 5
    plain = HDR + oracle.generate(0x1B00022, 0, n, 16, 12).tobytes()
    comp = bgzf_compress(plain)
    path = tmp_path / "big.gz"
    path.write_bytes(comp)
    idx, _, ranges = _run(driver, path, [1024, 65_536], _targets(len(comp), n, [7, 8, 9, 11, 13, 16, 21, 31]), shards=False)
    assert idx["rc"] == 0
    assert set(range(1, 10)) <= _check_ranges(idx, ranges, comp, plain)


def test_empty_blocks_the_eof_marker_and_a_header_across_blocks(ia, oracle, driver, tmp_path):
    n = 3 * REFILL + 11
    plain = HDR + oracle.generate(0x1B00021, 0, n, 16, 12).tobytes()
    edge = 32 + 24 * REFILL                                         # a range boundary of one refill per range, inside a block and on one
    cuts = [0, 7, 7, 32, 32, 5000, edge - 100, edge - 100, edge, edge, edge + 9000, 2 * edge, len(plain)]
    comp = b"".join(bgzf_compress(plain[a:z], eof=False) if z > a else dc.BGZF_EOF for a, z in zip(cuts, cuts[1:])) + dc.BGZF_EOF
    path = tmp_path / "e.gz"
    path.write_bytes(comp)
    idx, shards, ranges = _run(driver, path, SLOTS, _targets(len(comp), n))
    assert idx["rc"] == 0 and idx["lead"] == 3 and idx["head"] == 32
    assert sum(b[3] == 0 for b in idx["blocks"]) == 5
    _check_plans(ia, idx, shards, comp, plain)
    assert {1, 2, 4} <= _check_ranges(idx, ranges, comp, plain)       # (3 ranges would need ranges of 1.5 refills)


def test_a_file_the_index_refuses_plans_nothing(driver, tmp_path):
    path = tmp_path / "cut.gz"
    path.write_bytes(bgzf_compress(HDR + b"\x01" * 24 * 5000)[:-100])
    idx, shards, ranges = _run(driver, path, SLOTS, [1 << 30])
    assert idx["rc"] != 0 and not shards and not ranges
