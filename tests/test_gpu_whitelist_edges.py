"""The branches of k_whitelist.hip that random inputs do not reach (tests/test_gpu_whitelist.py draws its inputs): the
byte-wise class store, the scan of select over more than one round and select at its 2048-record unit seams, probe
sequences that wrap round the table or run through hundreds of slots, hits in the second ballot of the wave search, and
tiles in which every record misses.  Every comparison is byte for byte against tests/whitelist_np.py; the premises of the
crafted inputs (where a cluster lies, which neighbour number a hit has) are asserted on the CPU in
tests/test_whitelist_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import whitelist_np as wnp
from tests.test_gpu_whitelist import SIZES, _arena, _case, _check_untouched, _counts, _records, _whitelist

pytestmark = pytest.mark.gpu

TILE = 128                      # records per tile of ibu_k_correct (kTileRecs)
UNIT = 2048                     # records per unit of select (kSelUnit)
ROUND = UNIT * 1024 * 16        # records per iteration of ibu_k_select_scan (kScanBlock x kScanPer units): 33 554 432


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _correct_in_arena(ia, ctx, h, recs, mm, rskew, cskew, what):
    """correct_barcodes over `recs` at 24 n bytes `rskew` behind a 256-byte boundary with n class bytes `cskew` behind
    another, both out of a guarded arena -> (counts, records, classes) after the guard zones were checked."""
    n = len(recs)
    ar = _arena(ia, ctx, 24 * n, n)
    try:
        d = ar.carve(24 * n, rskew)
        d.upload(recs)
        d_cls = ar.carve(n, cskew)
        assert d.ptr % 16 == rskew and d_cls.ptr % 2 == cskew
        counts = ctx.correct_barcodes(h, d, n, mm, d_cls)
        ar.check(what)
        return counts, d.download(count=24 * n).view(wnp.REC), d_cls.download(np.uint8, n)
    finally:
        ar.free()


def _compare(got_counts, got, got_cls, recs, want, cls, bc_len):
    assert got_counts == _counts(cls)
    assert (got_cls == cls).all(), f"first wrong class at record {int(np.flatnonzero(got_cls != cls)[0])}"
    assert got.tobytes() == want.tobytes()
    _check_untouched(got, recs, cls, bc_len)


# ---- 1. the parity of the class pointer the tiled kernel gets ----------------------------------------------------------
def _head(n, rskew):            # an 8- but not 16-byte aligned record array peels one record into the tail kernel
    return min(n, 1) if rskew else 0


PARITY = [(n, rskew, cskew) for n in SIZES for rskew in (0, 8) for cskew in (0, 1)]
_TILED = [(n, r, c) for n, r, c in PARITY if (n - _head(n, r)) // TILE > 0]          # the cases in which ibu_k_correct runs
assert {(c + _head(n, r)) % 2 for n, r, c in _TILED} == {0, 1}, "both parities of (class skew + peeled head)"
assert {(r, c) for n, r, c in _TILED if (c + _head(n, r)) % 2} == {(0, 1), (8, 0)}, "the byte-wise store: both ways to it"


@pytest.mark.parametrize("n,rskew,cskew", PARITY)
def test_class_pointer_parity(ia, ctx, n, rskew, cskew):
    """ibu_k_correct stores two class bytes as one 16-bit word where its class pointer (d_class + peeled head) is even and as
    two bytes where it is odd: records aligned with d_class odd, and records skewed by 8 with d_class even."""
    bc_len = 16
    wl, recs, want, cls = _case(bc_len, 1000)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    with _whitelist(ia, ctx, wl, bc_len) as h:
        got = _correct_in_arena(ia, ctx, h, recs, 1, rskew, cskew, f"correct n={n} records +{rskew} classes +{cskew}")
    _compare(*got, recs, want, cls, bc_len)


# ---- 2. select at its unit seams and over several rounds of the scan ---------------------------------------------------
SEAMS = [2047, 2048, 2049, 4095, 4096, 4097, 16 * UNIT - 1, 16 * UNIT + 1]   # (16 units: what one thread of the scan sums)


@functools.lru_cache(maxsize=None)
def _seam_case(n):
    rng = np.random.default_rng(0x1B00700 + n)
    cls = rng.choice(np.array([0, 1, 2, 3, 0, 0, 1, 4, 7, 8, 200, 255], np.uint8), n)
    if n >= 2 * UNIT - 1:
        cls[:UNIT] = 2                                   # a whole unit with nothing / everything kept
    if n >= 16 * UNIT - 1:
        cls[3 * UNIT:5 * UNIT] = 0
        cls[9 * UNIT:10 * UNIT] = 3
    cls[n - 1] = 0                                       # the record behind the seam of n = 2048 k + 1
    return _records(rng, rng.integers(0, 1 << 32, n, dtype=np.uint64)), cls


@pytest.mark.parametrize("keep", range(16))
@pytest.mark.parametrize("n", SEAMS)
def test_select_at_unit_seams(ia, ctx, n, keep):
    recs, cls = _seam_case(n)
    want = recs[np.isin(cls, [c for c in range(4) if (keep >> c) & 1])]
    ar = _arena(ia, ctx, 24 * n, n, 24 * len(want))
    try:
        d, d_cls, d_out = ar.carve(24 * n), ar.carve(n, 1), ar.carve(24 * len(want))
        d.upload(recs)
        d_cls.upload(cls)
        k = C.c_size_t(99)
        ia._check(ia.lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, keep, None, 0, C.byref(k), None))           # size query
        assert k.value == len(want)
        k = C.c_size_t(99)
        ia._check(ia.lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, keep, d_out.ptr if len(want) else None, len(want), C.byref(k), None))
        ar.check(f"select n={n} keep={keep}")
        assert k.value == len(want)
        if len(want):
            assert d_out.download(count=24 * len(want)).tobytes() == want.tobytes()
        assert d.download(count=24 * n).tobytes() == recs.tobytes() and (d_cls.download(np.uint8, n) == cls).all()     # inputs untouched
    finally:
        ar.free()


def _scan_rounds(n):
    units = -(-n // UNIT)
    return -(-units // (1024 * 16))


BIG = [ROUND, ROUND + 1, 2 * ROUND + 2049]
assert ROUND == 33_554_432 and [_scan_rounds(n) for n in BIG] == [1, 2, 3]   # from the constants: none of them can become a one-round case unnoticed
assert BIG[-1] > 2 * 33_554_432


@functools.lru_cache(maxsize=1)
def _big_classes():
    """Class bytes for the largest n (the smaller ones take a prefix): the mix of the `mixed` fixture; round boundary 1 lies
    in a stretch of whole units of class 2 (three units before it, two behind), boundary 2 in one of class 0 (two before, one
    behind; the one record behind that is of class 3), so each boundary has nothing kept round it under one of the masks
    0b0011 / 0b1100 and everything under the other, and records are kept on both sides of both under either."""
    rng = np.random.default_rng(0x1B00701)
    cls = rng.choice(np.array([0, 1, 2, 3, 0, 0, 1, 4, 7, 8, 200, 255], np.uint8), BIG[-1])
    cls[ROUND - 3 * UNIT:ROUND + 2 * UNIT] = 2
    cls[2 * ROUND - 2 * UNIT:2 * ROUND + UNIT] = 0
    cls[2 * ROUND + UNIT:] = 3
    return cls


@pytest.mark.parametrize("n", BIG)
def test_select_across_scan_rounds(ia, ctx, n):
    """One iteration of ibu_k_select_scan covers 33 554 432 records: exactly one round, one round and one record, and three
    rounds.  Records carry index = i, the expected output is recs[keep]."""
    cls = _big_classes()[:n]
    recs = np.zeros(n, wnp.REC)
    recs["index"] = np.arange(n, dtype=np.uint64)
    recs["barcode"] = recs["index"] * np.uint64(0x9FB21C651E98DF25)
    recs["umi"] = ~recs["index"]
    d, d_cls = ctx.upload(recs), ctx.upload(cls)
    try:
        for keep in (0b0011, 0b1100):
            mask = np.isin(cls, [c for c in range(4) if (keep >> c) & 1])
            for b in range(1, _scan_rounds(n)):                                  # the premise, at every round boundary inside n
                lo, hi = mask[:b * ROUND], mask[b * ROUND:]
                assert lo.any() and (hi.any() or len(hi) == 1)                   # (one record behind the boundary: see below)
                around = np.concatenate([lo[-UNIT:], hi[:UNIT]])                     # a whole unit on either side, all alike
                assert around.all() or not around.any()
            if n == ROUND + 1:
                assert bool(mask[-1]) == (keep == 0b1100)                        # the second round's only record: kept under one mask
            want = recs[mask]
            k = C.c_size_t(99)
            ia._check(ia.lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, keep, None, 0, C.byref(k), None))
            assert k.value == len(want), (n, keep)
            out, k_out = ctx.select_records(d, d_cls, n, keep)
            try:
                assert k_out == len(want), (n, keep)
                got = out.download(wnp.REC, k_out)
            finally:
                out.free()
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, keep)
            del got, want
    finally:
        d.free(); d_cls.free()


# ---- 3. crafted tables: a cluster through the last slot into slot 0, chains of 512 and 1024 slots, contended builds ----
@functools.lru_cache(maxsize=2)
def _crafted(bc_len, kind, tripled):
    wl, keys, walkers, bc = wnp.crafted_table_case(bc_len, kind, tripled)
    recs = _records(np.random.default_rng(8), bc)
    want, cls, _ = wnp.correct_records(recs, wl, bc_len, 1)
    return wl, keys, recs, want, cls


@pytest.mark.parametrize("n", [129, 5121, 100_003])          # tail kernel and one tile; many tiles
@pytest.mark.parametrize("tripled", [False, True])
@pytest.mark.parametrize("kind", sorted(wnp.CRAFTED_TABLES))
@pytest.mark.parametrize("bc_len", [10, 16, 31, 32])
def test_crafted_tables(ia, ctx, bc_len, kind, tripled, n):
    wl, keys, recs, want, cls = _crafted(bc_len, kind, tripled)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    assert set(np.unique(cls)) >= {0, 1, 3}
    want0, cls0, _ = wnp.correct_records(recs, wl, bc_len, 0)
    with _whitelist(ia, ctx, wl, bc_len) as h:
        assert h.n_distinct == len(keys)
        got = _correct_in_arena(ia, ctx, h, recs, 1, 0, 0, f"{kind} bc_len={bc_len} n={n}")
        got0 = _correct_in_arena(ia, ctx, h, recs, 0, 8, 0, f"{kind} bc_len={bc_len} n={n}, no search")
    _compare(*got, recs, want, cls, bc_len)
    _compare(*got0, recs, want0, cls0, bc_len)


# ---- 4. hits in the first and the second ballot of the wave search, and the same barcodes in the lane-per-record search --
@pytest.mark.parametrize("bc_len,with_ones", [(21, True), (22, True), (23, True), (31, True), (32, True), (32, False)])
def test_hits_across_the_two_ballots(ia, ctx, bc_len, with_ones):
    """Every barcode of whitelist_np.ballot_case (a) spread through four full tiles, (b) as the first record of an 8-byte
    skewed array, which the tail kernel takes, and (c) in the n % 128 rest: the three must get the class and the barcode that
    numpy gives them, which is also what the case was built to give."""
    wl, bc, cls_built, low_built, specs = wnp.ballot_case(bc_len, with_ones)
    assert bc_len < 23 or any(s[0] != "ones" and len(s) == 2 and min(s) >= 66 for s in specs), "a pair with both bases at or above 22"
    K, m = len(bc), wnp.mask(bc_len)
    rng = np.random.default_rng([9, bc_len])
    junk = rng.integers(1, 1 << 62, K, dtype=np.uint64) << np.uint64(2 * bc_len) if bc_len < 32 else np.zeros(K, np.uint64)
    both = np.concatenate([bc, bc | junk])                                       # every barcode plain and (below 32 bases) with junk bits
    rest_n = 2 * K + 5
    assert rest_n < TILE
    body = np.where(rng.random(4 * TILE) < 0.5, wl[rng.integers(0, len(wl), 4 * TILE)], wnp.random_codes(rng, bc_len, 4 * TILE))
    where_body = rng.permutation(4 * TILE)[:2 * K]
    body[where_body] = both
    rest = wnp.random_codes(rng, bc_len, rest_n)
    where_rest = rng.permutation(rest_n)[:2 * K]
    rest[where_rest] = both
    with _whitelist(ia, ctx, wl, bc_len) as h:
        for k in range(2 * K if bc_len < 32 else K):
            barcodes = np.concatenate([both[k:k + 1], body, rest])
            n = len(barcodes)
            assert (n - 1) // TILE == 4 and (n - 1) % TILE == rest_n
            recs = _records(rng, barcodes)
            want, cls, _ = wnp.correct_records(recs, wl, bc_len, 1)
            got_counts, got, got_cls = _correct_in_arena(ia, ctx, h, recs, 1, 8, k % 2, f"ballots bc_len={bc_len} head={k}")
            _compare(got_counts, got, got_cls, recs, want, cls, bc_len)
            at = np.concatenate([[0], 1 + where_body, 1 + 4 * TILE + where_rest])    # (b), (a), (c)
            which = np.concatenate([[k], np.arange(2 * K), np.arange(2 * K)]) % K
            assert (got_cls[at] == cls_built[which]).all()
            assert ((got["barcode"][at] & m) == low_built[which]).all()


# ---- 5. tiles in which every record misses ----------------------------------------------------------------------------
def test_tiles_in_which_every_record_misses(ia, ctx):
    """Four tiles without one exact record, classes 1, 2 and 3 in every position of the tile, among ordinary tiles: the wave
    search then takes all 64 lanes in turn for both of a lane's records."""
    bc_len = 16
    wl, pools = wnp.miss_case(bc_len)
    rng = np.random.default_rng(10)
    ntiles, all_miss = 12, (3, 4, 5, 8)
    n = ntiles * TILE + 37
    pick = lambda c, k: pools[c][rng.integers(0, len(pools[c]), k)]
    bc = np.where(rng.random(n) < 0.6, wl[rng.integers(0, len(wl), n)], np.where(rng.random(n) < 0.5, pick(1, n), pick(3, n)))
    pos = np.arange(TILE)
    for turn, t in enumerate(all_miss):
        want_cls = (pos + turn) % 3 + 1
        tile = np.empty(TILE, np.uint64)
        for c in (1, 2, 3):
            tile[want_cls == c] = pick(c, int((want_cls == c).sum()))
        bc[t * TILE:(t + 1) * TILE] = tile
    recs = _records(rng, wnp.with_junk(rng, bc, bc_len))
    want, cls, _ = wnp.correct_records(recs, wl, bc_len, 1)
    tiles = cls[:ntiles * TILE].reshape(ntiles, TILE)
    assert [t for t in range(ntiles) if (tiles[t] != 0).all()] == list(all_miss)          # and the other tiles are ordinary
    for p in range(TILE):
        assert set(tiles[list(all_miss), p].tolist()) == {1, 2, 3}, p
    with _whitelist(ia, ctx, wl, bc_len) as h:
        got = _correct_in_arena(ia, ctx, h, recs, 1, 0, 0, "all-miss tiles")              # aligned: tile t is records 128 t ..
    _compare(*got, recs, want, cls, bc_len)


@pytest.mark.parametrize("mm", [1, 0])
def test_every_record_misses(ia, ctx, mm):
    bc_len, n = 16, 100_003
    wl, pools = wnp.miss_case(bc_len)
    rng = np.random.default_rng(11)
    bc = np.concatenate([pools[c][rng.integers(0, len(pools[c]), n // 3 + 1)] for c in (1, 2, 3)])
    recs = _records(rng, wnp.with_junk(rng, rng.permutation(bc)[:n], bc_len))
    want, cls, counts = wnp.correct_records(recs, wl, bc_len, mm)
    assert counts["exact"] == 0 and (min(counts["corrected"], counts["ambiguous"], counts["unmatched"]) > n // 4 if mm else counts["unmatched"] == n)
    with _whitelist(ia, ctx, wl, bc_len) as h:
        got = _correct_in_arena(ia, ctx, h, recs, mm, 0, 0, f"every record misses, max_mismatches={mm}")
    _compare(*got, recs, want, cls, bc_len)
