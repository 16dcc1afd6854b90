"""The host half of the BGZF device load (ibu_amd/csrc/bgzf_plan.hpp): the index of a file's blocks and the plan of every shard, driven
through tests/cpp/test_bgzf_plan.cpp and checked here against ibu_bgzf_scan, ibu_shard_range and the bytes the files were written from.
Runs without a GPU."""
import gzip
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests.bgzf import bgzf_compress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = struct.pack("<IIIIQ8s", 0x21554249, 2, 16, 12, 0, b"\0" * 8)


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/test_bgzf_plan"])
    return os.path.join(ROOT, "tests", "cpp", "bin", "test_bgzf_plan")


def _run(driver, path, pieces_min):
    r = subprocess.run([driver, str(path), str(pieces_min)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    return lines[0], lines[1:]


def _block(b):
    return [b.comp_offset, b.comp_len, b.out_offset, b.out_len, b.crc32]


def _check_plans(ia, idx, plans, comp, plain):
    B = idx["blocks"]
    n = (len(plain) - 32) // 24
    assert len(plans) == 45
    for p in plans:
        k, i, lo, hi = p["n_shards"], p["shard"], p["lo"], p["hi"]
        assert (p["rec_first"], p["rec_first"] + p["num"]) == ia.shard_range(n, k, i)
        assert (lo, hi) == (32 + 24 * p["rec_first"], 32 + 24 * (p["rec_first"] + p["num"]))
        dev = range(p["dev_first"], p["dev_end"])
        assert idx["lead"] <= p["dev_first"] <= p["dev_end"] <= len(B)
        assert len(p["edges"]) <= 2 and not set(p["edges"]) & set(dev) and all(e >= idx["lead"] for e in p["edges"])
        for j in dev:                                               # no device block straddles lo or hi
            assert lo <= B[j][2] and B[j][2] + B[j][3] <= hi, (k, i, j)
        pieces = [(0, idx["head"])] + [(B[j][2], B[j][2] + B[j][3]) for j in list(p["edges"]) + list(dev)]
        cut = sorted((max(a, lo), min(z, hi)) for a, z in pieces if max(a, lo) < min(z, hi))
        at = lo                                                     # the pieces cut to [lo, hi) tile it exactly once
        for a, z in cut:
            assert a == at, (k, i, cut)
            at = z
        assert at == hi, (k, i, cut)
        if k == 1:
            assert (p["cbeg"], p["cend"]) == (0, len(comp))
        elif len(dev):
            assert (p["cbeg"], p["cend"]) == (B[dev[0]][0], B[dev[-1]][0] + B[dev[-1]][1])
        else:
            assert (p["cbeg"], p["cend"]) == (0, 0)
        assert p["crc"] == zlib.crc32(plain[lo:hi])               # the plan's pieces, inflated on the host, are the shard's bytes


def _index_both_ways(ia, driver, tmp_path, comp, plain, name="f.gz"):
    path = tmp_path / name
    path.write_bytes(comp)
    plain_idx, plain_plans = _run(driver, path, 1 << 62)
    idx, plans = _run(driver, path, 0)                              # the walk in pieces, whatever the file's size
    assert plain_idx["rc"] == 0 and idx["rc"] == 0 and not plain_idx["in_pieces"]
    blocks, consumed, out_bytes, rc = ia.bgzf_scan(comp)
    assert rc == 0 and consumed == len(comp) and out_bytes == len(plain) == idx["total"]
    assert idx["blocks"] == plain_idx["blocks"] == [_block(b) for b in blocks]
    assert (idx["lead"], idx["head"]) == (plain_idx["lead"], plain_idx["head"]) and plans == plain_plans
    return idx, plans


@pytest.mark.parametrize("block", [20, 4093, 0xFF00])
@pytest.mark.parametrize("n", [0, 1, 5, 777, 100_003])
def test_index_and_plans_tile_every_shard(ia, oracle, driver, tmp_path, block, n):
    plain = HDR + oracle.generate(0x1B00010 + n, 0, n, 16, 12).tobytes()
    for eof in (True, False):
        comp = bgzf_compress(plain, block=block, eof=eof)
        idx, plans = _index_both_ways(ia, driver, tmp_path, comp, plain)
        assert idx["lead"] == (2 if block == 20 else 1) and idx["head"] == min(len(plain), block * idx["lead"])
        _check_plans(ia, idx, plans, comp, plain)
        if len(idx["blocks"]) >= 64:                                # enough blocks for every piece to find its own
            assert idx["in_pieces"]


def test_empty_blocks_mid_file_and_a_header_across_blocks(ia, oracle, driver, tmp_path):
    plain = HDR + oracle.generate(0x1B00011, 0, 20_000, 16, 12).tobytes()
    cuts = [0, 7, 7, 32, 32, 5000, 70_000, 70_000, 70_000, 200_000, 300_000, len(plain)]
    comp = b"".join(bgzf_compress(plain[a:z], eof=False) if z > a else dc.BGZF_EOF for a, z in zip(cuts, cuts[1:])) + dc.BGZF_EOF
    idx, plans = _index_both_ways(ia, driver, tmp_path, comp, plain)
    assert idx["lead"] == 3 and idx["head"] == 32                   # 7 bytes, an empty block, 25 bytes: the header
    assert sum(b[3] == 0 for b in idx["blocks"]) == 5
    _check_plans(ia, idx, plans, comp, plain)


@pytest.mark.parametrize("kind", ["records", "decoys"])
def test_walk_in_pieces_is_taken_or_refused(ia, oracle, driver, tmp_path, kind):
    """"decoys": stored blocks of records whose bytes spell a bgzip header every 97 records — every piece's first guess is wrong, and
    the plain walk decides."""
    n = 60_000
    recs = oracle.generate(0x1B00012, 0, n, 16, 12)
    level = 1
    if kind == "decoys":
        level = 0
        raw = recs.view(np.uint8).reshape(n, 24)
        raw[::97] = np.frombuffer(bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x11, 0x22] + [0] * 6), np.uint8)
    plain = HDR + recs.tobytes()
    comp = bgzf_compress(plain, level=level)
    idx, plans = _index_both_ways(ia, driver, tmp_path, comp, plain)
    assert idx["in_pieces"] == (kind == "records")
    _check_plans(ia, idx, plans, comp, plain)


def test_index_refuses_what_the_reader_refuses(ia, oracle, driver, tmp_path):
    plain = HDR + oracle.generate(0x1B00013, 0, 50_000, 16, 12).tobytes()
    good = bgzf_compress(plain)
    blocks, _, _, _ = ia.bgzf_scan(good)
    bad_crc = bytearray(good)                                       # the first block, inflated on the host for the header
    struct.pack_into("<I", bad_crc, blocks[0].comp_offset + blocks[0].comp_len, blocks[0].crc32 ^ 1)
    cases = {
        "gzip": (gzip.compress(plain), "Niffler"),
        "plain": (plain, "Niffler"),
        "cut_trailer": (good[:-60], "Niffler"),
        "cut_middle": (good[:len(good) // 2], "Niffler"),
        "cut_header": (good[:7], "Niffler"),
        "empty": (b"", "Io"),
        "lead_crc": (bytes(bad_crc), "Niffler"),
        "map_size": (bgzf_compress(plain + b"\x01\x02\x03"), "InvalidMapSize"),
        "short": (bgzf_compress(HDR[:20]), "Io"),
        "magic": (bgzf_compress(b"\0" * 32 + plain[32:]), "InvalidMagicNumber"),
        "bc_len": (bgzf_compress(struct.pack("<IIIIQ8s", 0x21554249, 2, 0, 12, 0, b"\0" * 8)), "InvalidBarcodeLength"),
    }
    for name, (data, want) in cases.items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        for pieces_min in (0, 1 << 62):
            idx, plans = _run(driver, path, pieces_min)
            assert ia.lib.ibu_status_name(idx["rc"]).decode() == want and not plans, (name, idx["rc"])
