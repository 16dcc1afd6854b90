"""The census of the sort (ibu_k_sort_census, ibu_k_sort_census_tail, the census inside ibu_k_sort_compress) and the sorted check,
one defect at a time: a base that is sorted and in index order gets ONE pair of neighbours out of order — or one record with a bit
no other record has — at every row where the launcher's split (peeled head row | 128-record tiles | rest) or a tile has a seam, and
the flags and words must be those of the plain statement (tests/census_np.py).  Then the three decisions the sort takes from them:
"already sorted", "in index order: no index passes", "this byte does not vary" — end to end against the oracle's sort.

The array is uploaded once per (n, alignment); a case overwrites its few records on the device, runs the calls and restores them."""
import ctypes as C

import numpy as np
import pytest

from tests import census_np as cn
from tests import keyplan_np as kp

pytestmark = pytest.mark.gpu

SEED = 0x1B00C5
OFFSETS = (0, 24)                                            # 24: an odd record of a larger buffer — 8- but not 16-byte aligned, one row is peeled
SAMPLE = 32_768                                              # the speculation's sample ranges: the first, middle and last 32 768 rows


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx24(ia):
    """Neither compact keys nor prefix + finish: the plain 24-byte passes, whose pass list skips the index digits on the census' word."""
    c = ia.Context(0)
    c.set_option("sort_compact", 0)
    c.set_option("sort_hybrid", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_guess(ia):
    """Speculation from 131 072 records on, plain element passes behind it (as the fixture of that name in test_gpu_sort.py)."""
    c = ia.Context(0)
    c.set_option("sort_guess", 131_072)
    c.set_option("sort_hybrid", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(ia, ctx):
    """hipDeviceProp_t::multiProcessorCount of device 0 — the number the library sizes its grids from — asked of the HIP runtime
    the library is linked to: a symbol looked up on the library's handle is found in its dependencies."""
    multiprocessor_count = 63                                # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h; part of the runtime's ABI)
    n = C.c_int(0)
    assert ia.lib.hipDeviceGetAttribute(C.byref(n), C.c_int(multiprocessor_count), C.c_int(0)) == 0
    assert 8 <= n.value <= 1024 and n.value % 8 == 0, n.value   # eight XCDs
    return n.value


@pytest.fixture
def own():
    """own(x) hands x back and frees it when the test ends, however it ends."""
    held = []

    def keep(x):
        held.append(x)
        return x

    yield keep
    for x in held:
        x.free()


class DeviceArray:
    """A clean base on the device, at `offset` bytes into its buffer."""

    def __init__(self, ia, ctx, n, offset, seed=None):
        self.ia, self.ctx, self.n, self.offset = ia, ctx, n, offset
        self.base = cn.Base(cn.clean_base(n, n if seed is None else seed))
        self.buf = ctx.alloc(24 * (n + 2))
        self.ptr = self.buf.ptr + offset
        self.write(0, self.base.recs)

    def write(self, row, recs):
        a = np.ascontiguousarray(recs)
        rc = self.ia.lib.ibu_memcpy_h2d(self.ctx._c, C.c_void_p(self.ptr + 24 * row), a.ctypes.data_as(C.c_void_p), a.nbytes, None)
        assert rc == 0
        self.ctx.synchronize()

    def check(self, patch, label, failures):
        """The census and the sorted check of the base with `patch` applied, against the statement; what differs goes to `failures`."""
        want = self.base.expect(patch)
        lo, win = self.base.window(patch)
        self.write(lo, win)
        try:
            got = self.ctx.census(self.ptr, self.n)
            srt = self.ctx.is_sorted(self.ptr, self.n)
        finally:
            self.write(lo, self.base.recs[lo:lo + len(win)])
        for key in ("index_drops", "order_drops", "or", "and"):
            if got[key] != want[key]:
                shown = ([hex(v) for v in got[key]], [hex(v) for v in want[key]]) if key in ("or", "and") else (got[key], want[key])
                failures.append(f"{label}: {key} is {shown[0]}, the statement says {shown[1]}")
        if srt != (not want["order_drops"]):
            failures.append(f"{label}: is_sorted is {srt}")
        return got, want

    def free(self):
        self.buf.free()


def _report(failures, cases):
    assert not failures, f"{len(failures)} of {cases} cases differ:\n" + "\n".join(failures[:40])


def _check_plan(ia, got, want, label, failures):
    plan, ref = ia.key_plan(got["or"], got["and"]), kp.Plan(want["or"], want["and"])
    if (plan.k, plan.index_bytes, [int(b) for b in plan.base]) != (ref.k, ref.index_bytes, ref.base):
        failures.append(f"{label}: key plan k={plan.k} index_bytes={plan.index_bytes}, the statement says k={ref.k} index_bytes={ref.index_bytes}")


# ---- the census and the sorted check -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n", cn.SMALL_SIZES)
def test_one_defect_at_every_seam(ia, ctx, own, n, offset):
    """Every kind of defect (census_np.plant) on the pair in front of every seam row of n rows, at both alignments: both flags, the
    sorted check and the words are the statement's — a flag must rise for the one pair that is out of order and must stay down next
    to a near miss (equal records, a lower field falling while a higher one rises)."""
    arr = own(DeviceArray(ia, ctx, n, offset))
    failures, cases = [], 0
    got, want = arr.check({0: tuple(int(arr.base.recs[f][0]) for f in kp.FIELDS)}, f"n={n} offset={offset} undamaged", failures)
    assert (want["index_drops"], want["order_drops"]) == (False, False)
    for p, name in cn.seams(n, offset == 24):
        for kind in cn.KINDS:
            patch = cn.plant(arr.base.recs, p, kind)
            _, want = arr.check(patch, f"n={n} offset={offset} row {p} ({name}) kind {kind}", failures)
            assert (want["index_drops"], want["order_drops"]) == cn.KIND_FLAGS[kind]
            cases += 1
    assert cases == len(cn.seams(n, offset == 24)) * len(cn.KINDS) > 0
    _report(failures, cases)


def _later_tiles(ntiles, cus):
    """The second and third tile of some waves' walks: wave w of a grid of G waves takes tiles w, w + G, w + 2 G.  G is
    cus * resident workgroups * 4; the launcher caps the resident workgroups at 7 and takes fewer if the kernel's occupancy is lower,
    so every count from 1 to 7 is named — whichever the grid has, waves 0 and 3 have both their later tiles here — and, for the full
    grid of 7, the last wave that walks three tiles."""
    tiles = set()
    for blocks in range(1, 8):
        grid_waves = cus * blocks * 4
        for w in (0, 3):
            tiles |= {w + grid_waves, w + 2 * grid_waves}
    grid_waves = cus * 7 * 4
    w = min(grid_waves - 1, ntiles - 1 - 2 * grid_waves)
    assert 0 <= w
    tiles |= {w + grid_waves, w + 2 * grid_waves}
    assert max(tiles) < ntiles
    return tiles


def _walk_tiles(ntiles, cus):
    """Tiles of the large array whose front seam gets the defects: the first and last four, every 97th in between, and the later
    tiles of some waves' walks."""
    return set(range(4)) | set(range(ntiles - 4, ntiles)) | set(range(4, ntiles - 4, 97)) | _later_tiles(ntiles, cus)


@pytest.mark.parametrize("offset", OFFSETS)
def test_one_defect_at_the_tile_seams_of_a_three_tile_walk(ia, ctx, own, cus, offset):
    """A grid of resident waves (at most 7 workgroups of 4 waves per CU) over 15 625 tiles: every wave walks two tiles with the
    next one's loads in flight, the first waves three — the record in front of a tile travels with that prefetch."""
    n = cn.LARGE_SIZE
    head, main, _ = cn.split(n, offset == 24)
    # 7 workgroups per CU is the launcher's cap: the grid has AT MOST cus * 7 * 4 waves whatever the kernel's occupancy, so the bound
    # below guarantees a three-tile walk on any grid the launcher can choose (_later_tiles names such a walk's tiles for each)
    ntiles = main // cn.TILE
    assert ntiles > 2 * cus * 7 * 4, (ntiles, cus)           # else no wave walks three tiles on this device: choose a larger n
    arr = own(DeviceArray(ia, ctx, n, offset))
    rows = dict(cn.tile_seams(n, offset == 24, _walk_tiles(ntiles, cus)))
    rows.update(dict(cn.seams(n, offset == 24)))
    assert len(rows) >= 8 + (ntiles - 8) // 97 + 6
    failures, cases = [], 0
    arr.check({0: tuple(int(arr.base.recs[f][0]) for f in kp.FIELDS)}, f"n={n} offset={offset} undamaged", failures)
    for p, name in sorted(rows.items()):
        for kind in cn.KINDS:
            arr.check(cn.plant(arr.base.recs, p, kind), f"n={n} offset={offset} row {p} ({name}) kind {kind}", failures)
            cases += 1
    _report(failures, cases)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n", cn.SMALL_SIZES + (cn.LARGE_SIZE,))
def test_a_lone_outlier_bit_at_every_seam(ia, ctx, own, cus, n, offset):
    """One record with a bit that no other record has (barcode bit 61, umi bit 44, index bit 40), then one without a bit that every
    other record has — at the seam rows, row 0, the last row and the first row of every wave (the record the wave's accumulator is
    relative to): the OR / AND words exactly, and the key plan they give."""
    arr = own(DeviceArray(ia, ctx, n, offset))
    rows = dict(cn.outlier_rows(n, offset == 24))
    if n == cn.LARGE_SIZE:
        head, main, _ = cn.split(n, offset == 24)
        named = set(range(4)) | set(range(main // cn.TILE - 4, main // cn.TILE)) | _later_tiles(main // cn.TILE, cus)
        assert max(named) < main // cn.TILE
        rows.update({head + cn.TILE * t: f"tile {t}" for t in named})
    failures, cases = [], 0
    for row, name in sorted(rows.items()):
        for f in kp.FIELDS:
            for clear in (False, True):
                label = f"n={n} offset={offset} row {row} ({name}) {f} bit {'cleared' if clear else 'set'}"
                got, want = arr.check(cn.plant_bit(arr.base.recs, row, f, clear), label, failures)
                _check_plan(ia, got, want, label, failures)
                cases += 1
    assert cases == 6 * len(rows) and {0, n - 1} <= set(rows)
    _report(failures, cases)


# ---- the shortcuts of the sort, end to end -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "24-byte passes"])
@pytest.mark.parametrize("offset", OFFSETS)
def test_sort_shortcuts_with_one_defect_at_every_seam(ia, ctx, ctx24, own, oracle, capfd, offset, which):
    """"Already sorted" returns the input untouched and "in index order" leaves the index passes out: with one pair out of order at
    a seam row the sort must still give the oracle's bytes; the undamaged base, and a base whose only defect is an index that falls
    where the barcode rises (sorted, not in index order), come back as they were, and the trace says why."""
    c = ctx if which == "default" else ctx24
    n = 1 + 3 * 128 + 37
    arr = own(DeviceArray(ia, c, n, offset))
    tmp = own(c.alloc(24 * (n + 2)))
    failures, cases = [], 0

    def sort(recs):
        arr.write(0, recs)
        capfd.readouterr()
        c.sort_records(arr.ptr, tmp.ptr + offset, n)
        c.synchronize()
        return ia.DeviceBuffer.wrap(c, arr.ptr, 24 * n).download().tobytes(), capfd.readouterr().err

    got, trace = sort(arr.base.recs)
    assert got == arr.base.recs.tobytes() and f"n={n} already sorted" in trace, trace
    for p, name in cn.seams(n, offset == 24):
        for kind in ("1", "3", "4", "2"):
            recs = cn.apply(arr.base.recs, cn.plant(arr.base.recs, p, kind))
            got, trace = sort(recs)
            cases += 1
            if got != oracle.sort_records(recs).tobytes():
                failures.append(f"offset={offset} row {p} ({name}) kind {kind}: not the oracle's order; {trace.strip()}")
            if kind == "2" and (got != recs.tobytes() or "already sorted" not in trace):
                failures.append(f"offset={offset} row {p} ({name}) kind 2: sorted input was not passed through; {trace.strip()}")
            if kind != "2" and "already sorted" in trace:
                failures.append(f"offset={offset} row {p} ({name}) kind {kind}: taken for sorted")
    _report(failures, cases)


# ---- the census inside the compress pass (the speculative sort) --------------------------------------------------------------------
def _tied_records(oracle, n, lens, seed):
    """Records in index order that are not sorted, every key byte of the widths varying, (barcode, umi) from a pool of 4000 pairs: ties
    that the index decides."""
    recs = oracle.generate(SEED + seed, 0, n, *lens)
    rng = np.random.default_rng(seed)
    rng.shuffle(recs)
    pick = rng.integers(0, 4000, n)
    recs["barcode"], recs["umi"] = recs["barcode"][:4000][pick], recs["umi"][:4000][pick]
    recs["index"] = np.arange(n, dtype=np.uint64)
    return recs


def _sample_ranges(n):
    return [(s, s + SAMPLE) for s in (0, (n // 2) & ~1, (n - SAMPLE) & ~1)]


@pytest.mark.parametrize("lens", [(16, 12), (32, 12)])       # 10 varying bytes: 12-byte elements; 14: 16-byte elements
def test_census_of_the_compress_pass_at_its_tile_seams(ia, ctx_guess, own, oracle, capfd, lens):
    """The speculative sort compresses on a plan guessed from three sample ranges and takes the exact census in the same pass
    (ibu_k_sort_compress<true>, its own copy of the tile logic).  Defects where no sample looks, on tile seams of that pass: an index
    that falls between equal (barcode, umi) must bring the index passes back ("first_digit_guess=miss"), a bit in a byte the samples
    saw constant must be noticed ("guess did not cover") — and the result is the oracle's either way.  The undamaged input keeps its
    index passes skipped ("first_digit_guess=hit").
    The main/rest seam lies in the last sample range at every n (the rest is shorter than a tile), so the samples see a defect there
    themselves and the trace wording above cannot come.  For that row the assertion is the WEAKER one: the oracle's bytes, and that
    the compact path ran ("path=compact", which "path=compact-speculated" contains as well) — a census that misses the pair or the
    bit still gives wrong bytes there."""
    n = 200_064 + 37
    base = _tied_records(oracle, n, lens, lens[0])
    plan = kp.Plan(*kp.census_words(base))
    assert (plan.k, plan.index_bytes) == ((10, 3) if lens[0] == 16 else (14, 3)) and cn.flags(base) == (False, True)
    head, main, rest = cn.split(n, False)
    unseen = [SAMPLE + cn.TILE * k for k in (1, 2, 3, 300)] + [SAMPLE + cn.TILE * 7 + 77]
    for p in unseen:
        assert not any(s <= q < e for s, e in _sample_ranges(n) for q in (p - 1, p)), p
    assert all(p % cn.TILE == 0 for p in unseen[:-1]) and unseen[-1] % cn.TILE not in (0, 1, 64, 127)
    seen = head + main
    assert rest and any(s <= seen - 1 and seen < e for s, e in _sample_ranges(n))
    pristine, work, tmp = own(ctx_guess.upload(base)), own(ctx_guess.alloc(24 * n)), own(ctx_guess.alloc(24 * n))
    failures, cases = [], 0

    def sort(patch):
        recs = cn.apply(base, patch)
        ctx_guess.copy(work, pristine, 24 * n)
        for row, r in patch.items():
            ia.DeviceBuffer.wrap(ctx_guess, work.ptr + 24 * row, 24).upload(recs[row:row + 1])
        capfd.readouterr()
        ctx_guess.sort_records(work, tmp, n)
        ctx_guess.synchronize()
        trace = capfd.readouterr().err
        return work.download(count=24 * n).tobytes() == oracle.sort_records(recs).tobytes(), trace

    ok, trace = sort({})
    assert ok and f"path=compact-speculated element_bytes={12 if plan.k <= 12 else 16} passes={plan.k - plan.index_bytes} first_digit_guess=hit" in trace, trace
    for p in unseen + [seen]:
        a = base[p - 1]
        cases_here = [("index falls between equal keys", {p: (int(a["barcode"]), int(a["umi"]), int(a["index"]) - 1)},
                       "first_digit_guess=miss" if p != seen else "path=compact-speculated"),
                      ("umi bit 44", {p: (int(base["barcode"][p]), int(base["umi"][p]) | 1 << 44, int(base["index"][p]))},
                       "guess did not cover" if p != seen else "path=compact"),
                      ("index bit 40", {p: (int(base["barcode"][p]), int(base["umi"][p]), int(base["index"][p]) | 1 << 40)},
                       "guess did not cover" if p != seen else "path=compact")]
        for what, patch, expect in cases_here:
            ok, trace = sort(patch)
            cases += 1
            if not ok:
                failures.append(f"lens={lens} row {p} {what}: not the oracle's order; {trace.strip()}")
            if expect not in trace:
                failures.append(f"lens={lens} row {p} {what}: no '{expect}' in the trace; {trace.strip()}")
    _report(failures, cases)


# ---- the census inside the partition pass (the sort over several shards) -----------------------------------------------------------
@pytest.mark.parametrize("compact", [True, False])
def test_partition_pass_sees_one_record_at_a_tile_seam(ia, oracle, compact):
    """Two shards in index order with ties on (barcode, umi) and constant index bits from 32 up; ONE record of the second shard, on a
    tile seam that no sample range contains, has an index below its predecessor's with bit 40 set — a byte the sampled plan takes for
    constant.  The partition pass (its compress kernel takes the exact census) must notice: the global order is the oracle's.  Also on
    the form that sorts first (sort_compact = 0 on the first context)."""
    counts = [200_003, 150_001]
    total = sum(counts)
    recs = _tied_records(oracle, total, (16, 12), 55)
    recs["index"] |= np.uint64(1 << 41)
    p = counts[0] + SAMPLE + 3 * cn.TILE                      # row SAMPLE + 384 of the second shard: the first row of its tile 259
    assert not any(s <= q < e for s, e in _sample_ranges(counts[1]) for q in (p - counts[0] - 1, p - counts[0]))
    recs[p] = (recs["barcode"][p - 1], recs["umi"][p - 1], (int(recs["index"][p]) & ~(1 << 41)) | 1 << 40)
    assert recs["index"][p] < recs["index"][p - 1] and cn.drop_rows(recs)[0].tolist() == [p]
    assert kp.Plan(*kp.census_words(np.delete(recs, p))).k == 10 and kp.Plan(*kp.census_words(recs)).k == 11
    want = oracle.sort_records(recs).tobytes()
    ctxs = [ia.Context(0) for _ in counts]
    try:
        shards, at = [], 0
        for c, n in zip(ctxs, counts):
            d, t = c.alloc(24 * total), c.alloc(24 * total)   # (Context.close below frees what the context still owns)
            d.upload(recs[at:at + n])
            shards.append((d, t, n, total))
            at += n
        if not compact:
            ctxs[0].set_option("sort_compact", 0)
        out = ia.Context.sort_records_contexts(ctxs, shards)
        assert sum(out) == total
        assert b"".join(shards[k][0].download(count=24 * out[k]).tobytes() for k in range(len(counts))) == want
    finally:
        for c in ctxs:
            c.close()
