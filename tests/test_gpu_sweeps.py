"""The persistent sweep of the tiled kernels with waves that sweep SEVERAL tiles (kcommon.hpp: tile_range, sweep_tiles, and the loops
written out in k_decode.hip / k_encode.hip): every sweeping kernel, byte for byte against the reference its own test uses.

A launcher starts ceil(ntiles / 4) workgroups until the cap of cus x blocks_per_cu is reached, so at the sizes of the other files
nearly every wave has one tile and the loop that runs at production sizes (the next tile's loads in flight, two register sets taking
turns, the wave's LDS slice reused, the per-wave tallies carried from tile to tile) is hardly entered.  Here the contexts have
blocks_per_cu = 1, the tile size of a kernel is read from its trace line (option trace_rows), and the number of tiles comes from
tests/sweep_np.py: 8 (3 wpx + 38) - 3 tiles, wpx the waves of an XCD — on 256 CUs 3373 tiles, 38 waves of every XCD sweep four
tiles and the others three, the sweep ends in phase A for some waves and in phase B for others, and the last XCD's part is three
tiles short.  The kernels with 1024-row units or whose numpy statement is slow take the smaller shape (waves of one and two
tiles).  Every case asserts from the trace of the real call that exactly these tiles ran tiled, and from the mirror that some wave has
four (or two) tiles: whether the sweep iterates is decided by the test, not by chance.  Every case runs on a 16-byte aligned base
and on one whose arrays need one row peeled, which moves every tile seam by one.

What the traces give on an MI355X (256 CUs; 3373 tiles, 723 waves with three and 301 with four), rows per tile -> n:
  128 -> 431 821: deserialize, serialize, swap_umi_index, reduce, generate, census, compress, correct, abundance add, the feature
         class kernel, every encode, decode with a runtime length or fewer than 20 bases, pack 32 (copy: 3373 tiles of 4 KiB);
  256 -> 863 565: decode (16,12) and (32,32), unpack 13 and 32, pack 12, 13 and 16 (expand: two sub-tiles per tile, 3373 tiles);
  512 -> 1 727 053: unpack 12 and 16, pack 5;
  1024 -> 1 356 877 (1325 units, 723 waves with one and 301 with two): resolve — whitelist_np.correct_records needs 19 s on the
         3.45 M records of the larger shape and 2.6 s on these; no other reference needs more than a second;
  the unit loops (select, matrix rows, matrix text): 1325 units of 2048, n = 2 711 629.
Three deliberate defects, each in bounds, were built once and run against this file: phase B of sweep_tiles working on the other
register set fails every case of a kernel that goes through sweep_tiles (28 of 67: all but decode, encode, pack and the unit loops);
the last XCD's range ending one tile early fails every case of a kernel that goes through tile_range (62: all but the unit loops
and the probe of the tile sizes); a BadRows tally cleared at the top of every tile fails the 14 bad-row cases.

Out of scope: the merge kernel (tests/test_gpu_merge.py sets blocks_per_cu = 1 itself); the segment walk (runs_walk.hpp: one wave
per segment, no persistent sweep); the sort's scatter and finishing kernels (not capped by blocks_per_cu); the capped_grid
kernels."""
import ctypes as C

import numpy as np
import pytest

from tests import count_np as cnp
from tests import feature_np as fnp
from tests import keyplan_np as kp
from tests import mtx_np
from tests import resolve_np as rnp
from tests import sweep_np as sw
from tests import whitelist_np as wnp
from tests.test_gpu_count import _arena, _p, _swap

pytestmark = pytest.mark.gpu

SEED = 0x1B005EE
REST = 77                                                        # rows behind the last tile: the tail kernel's
SKEWS = [0, 8]                                                   # the record base: 16-byte aligned / 8 bytes behind (one row is peeled)
UNIT = 2048                                                      # k_whitelist.hip kSelUnit, k_matrix.hip kMtxUnit: entries per unit of a unit loop
COPY_TILE = 4096                                                 # k_records.hip ibu_k_copy: bytes per tile
CHOSEN = []                                                      # one line per case saying what was chosen; printed when the module is done (pytest -s)


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


def _context(ia, **options):
    c = ia.Context(0)
    c.set_option("blocks_per_cu", 1)                             # the grid of every tiled kernel: min(ceil(ntiles / 4), cus)
    for k, v in options.items():
        c.set_option(k, v)
    return c


@pytest.fixture(scope="module")
def ctx(ia):
    c = _context(ia)
    yield c
    c.close()
    print("\n" + "\n".join(sorted(set(CHOSEN))))


@pytest.fixture(scope="module")
def ctx_msb(ia):
    c = _context(ia, base_order=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(ia, ctx):
    """hipDeviceProp_t::multiProcessorCount of device 0 (what torch calls multi_processor_count), asked of the HIP runtime the library
    is linked to — the number the library sizes its grids from."""
    n = C.c_int(0)
    assert ia.lib.hipDeviceGetAttribute(C.byref(n), C.c_int(63), C.c_int(0)) == 0   # hipDeviceAttributeMultiprocessorCount
    assert 8 <= n.value <= 1024, n.value
    return n.value


@pytest.fixture(scope="module")
def full(oracle, cus):
    """Full-range records (bits above 2 len must be ignored) for the largest case: the 3/4 shape at 512-row tiles."""
    recs = oracle.generate(SEED, 0, sw.choose_ntiles(cus) * 512 + REST + 16, 32, 32)
    recs.setflags(write=False)
    return recs


def _traced(ctx, capfd, call):
    """call() with trace_rows on -> (its result, the `ibu rows:` lines of its launches as dicts of ints)."""
    ctx.synchronize()
    capfd.readouterr()
    ctx.set_option("trace_rows", 1)
    try:
        out = call()
        ctx.synchronize()
    finally:
        ctx.set_option("trace_rows", 0)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("ibu rows:")]
    return out, [{k: int(v) for k, v in (kv.split("=") for kv in ln.split()[2:])} for ln in lines]


def _probe(ctx, capfd, call):
    """The tile size and the peeled head of a kernel, from the trace of one call over 16 rows of tiny buffers with the alignment of
    the real ones."""
    _, rows = _traced(ctx, capfd, call)
    assert rows and len({(r["tile"], r["head"]) for r in rows}) == 1, rows
    assert rows[0]["n"] == 16 and rows[0]["tiled"] == 0
    return rows[0]["tile"], rows[0]["head"]


def _shape(what, cus, tile, head, base=3):
    """-> (n, ntiles, plan) for a kernel of `tile` rows per tile; CHOSEN gets a line that says what was chosen."""
    ntiles = sw.choose_ntiles(cus, base)
    plan = sw.sweep_plan(cus, 1, ntiles)
    hist = sw.histogram(plan)
    assert set(hist) == {base, base + 1} and max(map(len, plan)) == base + 1, hist
    n = head + ntiles * tile + REST
    CHOSEN.append(f"sweep: {what}: tile={tile} head={head} ntiles={ntiles} n={n} tiles per wave {dict(sorted(hist.items()))}")
    return n, ntiles, plan


def _assert_tiled(rows, n, ntiles, head=None, count=1):
    """Every traced launch of the real call ran exactly `ntiles` tiles tiled."""
    assert len(rows) >= count, rows
    for r in rows:
        assert r["n"] == n and r["tiled"] == ntiles * r["tile"] and r["rest"] == REST, (r, ntiles)
        assert head is None or r["head"] == head, (r, head)


def _skew_of(length, skew):
    """Where a column of `length`-byte rows starts so that peeling one row aligns it (skew 8), or 0."""
    return (-length) % 16 if skew else 0


# ---- K1 / K1', the field exchange, reduce, generate, copy ------------------------------------------------------------
@pytest.mark.parametrize("skew", SKEWS)
def test_deserialize_serialize(ia, ctx, oracle, capfd, cus, full, skew):
    tiny = [ctx.alloc(24 * 16 + 16)] + [ctx.alloc(8 * 16 + 16) for _ in range(3)]
    tile, head = _probe(ctx, capfd, lambda: ctx.deserialize(tiny[0].ptr + skew, 16, *[t.ptr + skew for t in tiny[1:]]))
    assert _probe(ctx, capfd, lambda: ctx.serialize(*[t.ptr + skew for t in tiny[1:]], 16, tiny[0].ptr + skew)) == (tile, head)
    assert head == (1 if skew else 0)
    n, ntiles, plan = _shape("deserialize / serialize", cus, tile, head)
    recs = full[:n]
    want = oracle.deserialize(recs)
    ar = _arena(ia, ctx, 24 * n, 8 * n, 8 * n, 8 * n, 24 * n)
    try:
        d = ar.carve(24 * n, skew)
        cols = [ar.carve(8 * n, skew) for _ in range(3)]
        back = ar.carve(24 * n, skew)
        d.upload(recs)
        _, rows = _traced(ctx, capfd, lambda: (ctx.deserialize(d, n, *cols), ctx.serialize(*cols, n, back)))
        _assert_tiled(rows, n, ntiles, head, 2)
        ar.check("deserialize / serialize")
        for c, w in zip(cols, want):
            assert c.download(np.uint64, n).tobytes() == w.tobytes()
        assert back.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        ar.free()
        for t in tiny:
            t.free()


@pytest.mark.parametrize("skew", SKEWS)
def test_swap_out_of_place_and_in_place(ia, ctx, capfd, cus, full, skew):
    """dst == src: a wave owns whole tiles and a tile is in LDS before any of it is written, while the next tile's loads are in
    flight (k_records.hip) — the argument is about this loop."""
    tiny = ctx.alloc(24 * 16 + 16)
    tile, head = _probe(ctx, capfd, lambda: _swap(ia, ctx, ia.DeviceBuffer.wrap(ctx, tiny.ptr + skew, 24 * 16), ia.DeviceBuffer.wrap(ctx, tiny.ptr + skew, 24 * 16), 16))
    n, ntiles, plan = _shape("swap_umi_index", cus, tile, head)
    recs = full[:n]
    want = cnp.swap(recs)
    ar = _arena(ia, ctx, 24 * n, 24 * n)
    try:
        src, dst = ar.carve(24 * n, skew), ar.carve(24 * n, skew)
        src.upload(recs)
        _, rows = _traced(ctx, capfd, lambda: (_swap(ia, ctx, src, dst, n), _swap(ia, ctx, src, src, n)))
        _assert_tiled(rows, n, ntiles, head, 2)
        ar.check("swap")
        assert dst.download(count=24 * n).tobytes() == want.tobytes(), "out of place"
        assert src.download(count=24 * n).tobytes() == want.tobytes(), "in place"
        _swap(ia, ctx, src, src, n)
        ar.check("swap in place, again")
        assert src.download(count=24 * n).tobytes() == recs.tobytes(), "twice is the identity"
    finally:
        ar.free()
        tiny.free()


def _add_reduced(a, b):
    m = (1 << 64) - 1
    return {"count": a["count"] + b["count"], "sum": [(x + y) & m for x, y in zip(a["sum"], b["sum"])], "xor": [x ^ y for x, y in zip(a["xor"], b["xor"])]}


@pytest.mark.parametrize("skew", SKEWS)
def test_reduce_generate_copy(ia, ctx, oracle, capfd, cus, full, skew):
    tiny = ctx.alloc(24 * 16 + 16)
    tile, head = _probe(ctx, capfd, lambda: ctx.reduce(tiny.ptr + skew, 16))
    assert _probe(ctx, capfd, lambda: ctx.generate(1, 0, 16, 16, 12, tiny.ptr + skew)) == (tile, head)
    n, ntiles, plan = _shape("reduce / generate (copy: the same number of 4 KiB tiles)", cus, tile, head)
    nbytes = (8 if skew else 0) + ntiles * COPY_TILE + REST * 16 + 5   # a head of 8 bytes, ntiles tiles, 77 chunks, 5 bytes
    payload = np.random.default_rng(skew).integers(0, 256, nbytes, dtype=np.uint8)
    ar = _arena(ia, ctx, 24 * n, 24 * n, nbytes, nbytes)
    try:
        d, g, cs, cp = ar.carve(24 * n, skew), ar.carve(24 * n, skew), ar.carve(nbytes, skew), ar.carve(nbytes, skew)
        d.upload(full[:n])
        cs.upload(payload)
        # all seven totals (count, three wrapping sums, three XORs), accumulated over two calls: the second on rows 6 .. n
        (_, got), rows = _traced(ctx, capfd, lambda: (ctx.reduce(d, n, fetch=False), ctx.reduce(d.ptr + 24 * 6, n - 6, reset=False)))
        assert len(rows) == 2 and rows[0]["tiled"] == ntiles * tile and rows[0]["head"] == head and rows[1]["tiled"] >= (ntiles - 1) * tile, rows
        assert got == _add_reduced(oracle.reduce_records(full[:n]), oracle.reduce_records(full[6:n]))
        _, rows = _traced(ctx, capfd, lambda: ctx.generate(SEED, 7, n, 20, 7, g))
        _assert_tiled(rows, n, ntiles, head)
        ctx.copy(cp, cs, nbytes)
        ar.check("reduce / generate / copy")
        assert g.download(count=24 * n).tobytes() == oracle.generate(SEED, 7, n, 20, 7).tobytes()
        assert cp.download(count=nbytes).tobytes() == payload.tobytes() == cs.download(count=nbytes).tobytes()
    finally:
        ar.free()
        tiny.free()


# ---- the fused codec -------------------------------------------------------------------------------------------------
# (bc_len, umi_len, first base most significant, index column given): the lengths cover both tile sizes of k_decode.hip (two 128-
# record tiles per iteration where both lengths are specialised multiples of 4 with at least 20 bases, else one) and every kind of
# instantiation of k_encode.hip: both specialised, both at run time, one of each.
CODEC = [(16, 12, False, True), (16, 12, True, False), (32, 32, False, False), (32, 32, True, True), (15, 11, False, True),
         (15, 11, True, False), (8, 8, False, True), (12, 7, True, True), (9, 16, False, False)]
FIRST_INDEX = 10**12 + 5


class _CodecBuffers:
    """recs | bc | umi | idx | back carved for n rows, every array one peeled row behind a 16-byte boundary (skew 8) or on one; or,
    shard = k, all of them at row k of arrays that start on a boundary."""

    def __init__(self, ia, ctx, n, bc_len, umi_len, skew, shard=0):
        sizes = [24, bc_len, umi_len, 8, 24]
        self.ar = _arena(ia, ctx, *[s * (n + shard) for s in sizes])
        whole = [self.ar.carve(s * (n + shard), _skew_of(s, skew)) for s in sizes]
        self.recs, self.bc, self.umi, self.idx, self.back = [ia.DeviceBuffer.wrap(ctx, w.ptr + s * shard, s * n) for w, s in zip(whole, sizes)]

    def free(self):
        self.ar.free()


def _codec_case(ia, c, oracle, capfd, cus, full, lens, msb, with_idx, skew, shard=0):
    bc_len, umi_len = lens
    order = 1 if msb else 0
    tiny = _CodecBuffers(ia, c, 16, bc_len, umi_len, skew, shard)
    idx_of = lambda b: b.idx if with_idx else None
    dec_tile, head = _probe(c, capfd, lambda: c.decode_ascii(tiny.recs, 16, bc_len, umi_len, tiny.bc, tiny.umi, idx_of(tiny)))
    enc_tile, enc_head = _probe(c, capfd, lambda: c.encode_ascii(tiny.bc, tiny.umi, idx_of(tiny), 16, bc_len, umi_len, tiny.back))
    _status(ia, c)                                               # the tiny columns hold the arena's pattern, not bases
    tiny.free()
    assert enc_head == head and (shard or head == (1 if skew else 0)), (head, enc_head)
    seen = set()
    for tile in sorted({dec_tile, enc_tile}):
        n, ntiles, plan = _shape(f"decode / encode {lens} (decode tile {dec_tile}, encode tile {enc_tile})", cus, tile, head)
        recs = full[shard:shard + n]
        bc, umi, idx = oracle.decode_records(recs, bc_len, umi_len, order)
        b = _CodecBuffers(ia, c, n, bc_len, umi_len, skew, shard)
        try:
            b.recs.upload(recs)
            _, rows = _traced(c, capfd, lambda: c.decode_ascii(b.recs, n, bc_len, umi_len, b.bc, b.umi, idx_of(b)))
            if tile == dec_tile:
                _assert_tiled(rows, n, ntiles, head)
                seen.add("decode")
            b.ar.check(f"decode {lens}")
            assert b.bc.download(count=n * bc_len).tobytes() == bc.tobytes()
            assert b.umi.download(count=n * umi_len).tobytes() == umi.tobytes()
            if with_idx:
                assert b.idx.download(np.uint64, n).tobytes() == idx.tobytes()
            _, rows = _traced(c, capfd, lambda: c.encode_ascii(b.bc, b.umi, idx_of(b), n, bc_len, umi_len, b.back, first_index=FIRST_INDEX))
            c.codec_status()
            if tile == enc_tile:
                _assert_tiled(rows, n, ntiles, head)
                seen.add("encode")
            b.ar.check(f"encode {lens}")
            want, _, nb = oracle.encode_records(bc, umi, idx if with_idx else None, n, bc_len, umi_len, first_index=FIRST_INDEX, order=order)
            assert nb == 0 and b.back.download(count=24 * n).tobytes() == want.tobytes()
        finally:
            b.free()
    assert seen == {"decode", "encode"}
    return dec_tile, enc_tile


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("bc_len,umi_len,msb,with_idx", CODEC)
def test_decode_encode(ia, ctx, ctx_msb, oracle, capfd, cus, full, bc_len, umi_len, msb, with_idx, skew):
    _codec_case(ia, ctx_msb if msb else ctx, oracle, capfd, cus, full, (bc_len, umi_len), msb, with_idx, skew)


def test_decode_tile_sizes_are_all_met(ia, ctx, capfd):
    """The pairs of CODEC meet every tile size a decode or encode instantiation has: the traces of all 25 pairs of length classes
    (runtime, 8, 12, 16, 32) name no size that the pairs of CODEC do not."""
    tiny = _CodecBuffers(ia, ctx, 16, 32, 32, 0)
    sizes = {}
    for bc_len in (7, 8, 12, 16, 32):
        for umi_len in (7, 8, 12, 16, 32):
            d, _ = _probe(ctx, capfd, lambda: ctx.decode_ascii(tiny.recs, 16, bc_len, umi_len, tiny.bc, tiny.umi, tiny.idx))
            e, _ = _probe(ctx, capfd, lambda: ctx.encode_ascii(tiny.bc, tiny.umi, tiny.idx, 16, bc_len, umi_len, tiny.back))
            sizes[bc_len, umi_len] = (d, e)
    _status(ia, ctx)                                             # the tiny columns hold the arena's pattern, not bases
    tiny.free()
    cls = lambda length: length if length in (8, 12, 16, 32) else 7
    met = {sizes[cls(b), cls(u)] for b, u, _, _ in CODEC}
    assert {s[0] for s in sizes.values()} == {s[0] for s in met} and {s[1] for s in sizes.values()} == {s[1] for s in met}, sizes


@pytest.mark.parametrize("bc_len,umi_len,msb", [(16, 12, False), (15, 11, True)])
def test_decode_encode_of_a_shard_at_record_3(ia, ctx, ctx_msb, oracle, capfd, cus, full, bc_len, umi_len, msb):
    _codec_case(ia, ctx_msb if msb else ctx, oracle, capfd, cus, full, (bc_len, umi_len), msb, True, 0, shard=3)


# ---- the single-column codec -----------------------------------------------------------------------------------------
# 12 and 16: the four-tile unpack and the two-tile pack class; 32: the two-tile unpack and the one-tile pack; 13: the runtime path
COLUMN = [(12, False), (16, False), (32, False), (13, False), (16, True), (13, True)]


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("length,msb", COLUMN)
def test_unpack_pack(ia, ctx, ctx_msb, oracle, capfd, cus, full, length, msb, skew):
    c, order = (ctx_msb, 1) if msb else (ctx, 0)
    tiny = [c.alloc(8 * 16 + 32), c.alloc(length * 16 + 32)]
    at = [tiny[0].ptr + skew, tiny[1].ptr + _skew_of(length, skew)]
    unp_tile, head = _probe(c, capfd, lambda: c.unpack_2bit(at[0], 16, length, at[1]))
    pack_tile, pack_head = _probe(c, capfd, lambda: c.pack_2bit(at[1], 16, length, at[0]))
    _status(ia, c)
    for t in tiny:
        t.free()
    assert head == pack_head == (1 if skew else 0)
    for tile in sorted({unp_tile, pack_tile}):
        n, ntiles, plan = _shape(f"unpack / pack {length} (unpack tile {unp_tile}, pack tile {pack_tile})", cus, tile, head)
        codes = np.ascontiguousarray(full["umi"][:n])
        want = oracle.unpack_column(codes, length, order)
        ar = _arena(ia, c, 8 * n, length * n, 8 * n)
        try:
            d_codes, d_ascii, d_back = ar.carve(8 * n, skew), ar.carve(length * n, _skew_of(length, skew)), ar.carve(8 * n, skew)
            d_codes.upload(codes)
            _, rows = _traced(c, capfd, lambda: c.unpack_2bit(d_codes, n, length, d_ascii))
            if tile == unp_tile:
                _assert_tiled(rows, n, ntiles, head)
            ar.check(f"unpack {length}")
            assert d_ascii.download(count=length * n).tobytes() == want.tobytes()
            _, rows = _traced(c, capfd, lambda: c.pack_2bit(d_ascii, n, length, d_back))
            c.codec_status()
            if tile == pack_tile:
                _assert_tiled(rows, n, ntiles, head)
            ar.check(f"pack {length}")
            wcodes, _, nb = oracle.pack_column(want, n, length, order)
            assert nb == 0 and d_back.download(np.uint64, n).tobytes() == wcodes.tobytes()
        finally:
            ar.free()


# ---- bad rows: the per-wave tally over several tiles -----------------------------------------------------------------
def _bad_scenarios(plan, ntiles, tile):
    """Rows (relative to the first tiled row) that get an invalid base, chosen with the mirror: one wave that sweeps four tiles gets
    bad rows in its second and fourth tile only; then in its third tile only; then one row in the last tile of the short last XCD
    part.  A tally that is reset or overwritten from tile to tile loses rows of the first two."""
    w = sw.wave_with(plan, 4)
    last = sw.owner(plan, ntiles - 1)
    assert last[-1] == ntiles - 1 and len(last) >= 3
    return [("second and fourth tile", [w[1] * tile + r for r in (0, 5, tile - 1)] + [w[3] * tile + r for r in (1, tile // 2)]),
            ("third tile", [w[2] * tile + r for r in (2, tile - 2)]),
            ("last tile of the last part", [(ntiles - 1) * tile + tile - 1])]


def _status(ia, c):
    try:
        c.codec_status()
        return None, 0
    except ia.IbuError as e:
        assert e.kind == "InvalidBase"
        return e.first_bad, e.n_bad


def _poke(ia, c, buf, offset, value):
    ia.DeviceBuffer.wrap(c, buf.ptr + offset, 1).upload(np.array([value], np.uint8))


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("bc_len,umi_len,msb", [(16, 12, False), (15, 11, True), (32, 7, False)])
def test_encode_bad_rows_in_chosen_tiles_of_one_wave(ia, ctx, ctx_msb, oracle, capfd, cus, full, bc_len, umi_len, msb, skew):
    c, order = (ctx_msb, 1) if msb else (ctx, 0)
    tiny = _CodecBuffers(ia, c, 16, bc_len, umi_len, skew)
    tile, head = _probe(c, capfd, lambda: c.encode_ascii(tiny.bc, tiny.umi, tiny.idx, 16, bc_len, umi_len, tiny.back))
    _status(ia, c)
    tiny.free()
    n, ntiles, plan = _shape(f"encode ({bc_len}, {umi_len}) with bad rows", cus, tile, head)
    bc, umi, idx = oracle.decode_records(full[:n], bc_len, umi_len, order)
    b = _CodecBuffers(ia, c, n, bc_len, umi_len, skew)
    try:
        b.bc.upload(bc)
        b.umi.upload(umi)
        b.idx.upload(idx)
        for what, rows in _bad_scenarios(plan, ntiles, tile):
            rows = [head + r for r in rows]
            hb, hu = bc.copy().reshape(-1), umi.copy().reshape(-1)
            for k, r in enumerate(rows):                        # alternately a barcode byte and a UMI byte, first / last base
                col, length, dev = (hb, bc_len, b.bc) if k % 2 == 0 else (hu, umi_len, b.umi)
                at = r * length + (0 if k % 3 == 0 else length - 1)
                col[at] = ord("N")
                _poke(ia, c, dev, at, ord("N"))
            want, fb, nb = oracle.encode_records(hb, hu, idx, n, bc_len, umi_len, order=order)
            assert (fb, nb) == (rows[0], len(rows))
            _, traced = _traced(c, capfd, lambda: c.encode_ascii(b.bc, b.umi, b.idx, n, bc_len, umi_len, b.back))
            _assert_tiled(traced, n, ntiles, head)
            assert _status(ia, c) == (fb, nb), what
            assert b.back.download(count=24 * n).tobytes() == want.tobytes(), what   # the fields of a bad row are zero
            for k, r in enumerate(rows):                        # put the valid bytes back
                col, length, dev = (bc.reshape(-1), bc_len, b.bc) if k % 2 == 0 else (umi.reshape(-1), umi_len, b.umi)
                at = r * length + (0 if k % 3 == 0 else length - 1)
                _poke(ia, c, dev, at, int(col[at]))
        b.ar.check("encode with bad rows")
    finally:
        b.free()


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("length,msb", [(12, False), (32, False), (13, True), (5, False)])
def test_pack_bad_rows_in_chosen_tiles_of_one_wave(ia, ctx, ctx_msb, oracle, capfd, cus, full, length, msb, skew):
    c, order = (ctx_msb, 1) if msb else (ctx, 0)
    tiny = [c.alloc(8 * 16 + 32), c.alloc(length * 16 + 32)]
    tile, head = _probe(c, capfd, lambda: c.pack_2bit(tiny[1].ptr + _skew_of(length, skew), 16, length, tiny[0].ptr + skew))
    _status(ia, c)
    for t in tiny:
        t.free()
    n, ntiles, plan = _shape(f"pack {length} with bad rows", cus, tile, head)
    col = oracle.unpack_column(np.ascontiguousarray(full["barcode"][:n]), length, order).reshape(-1)
    ar = _arena(ia, c, length * n, 8 * n)
    try:
        d_ascii, d_codes = ar.carve(length * n, _skew_of(length, skew)), ar.carve(8 * n, skew)
        d_ascii.upload(col)
        for what, rows in _bad_scenarios(plan, ntiles, tile):
            rows = [head + r for r in rows]
            host = col.copy()
            for k, r in enumerate(rows):
                at = r * length + (0, length - 1, length // 2)[k % 3]
                host[at] = (ord("N"), 0, 0xC1)[k % 3]
                _poke(ia, c, d_ascii, at, int(host[at]))
            want, fb, nb = oracle.pack_column(host, n, length, order)
            assert (fb, nb) == (rows[0], len(rows))
            _, traced = _traced(c, capfd, lambda: c.pack_2bit(d_ascii, n, length, d_codes))
            _assert_tiled(traced, n, ntiles, head)
            assert _status(ia, c) == (fb, nb), what
            assert d_codes.download(np.uint64, n).tobytes() == want.tobytes(), what
            for k, r in enumerate(rows):
                at = r * length + (0, length - 1, length // 2)[k % 3]
                _poke(ia, c, d_ascii, at, int(col[at]))
        ar.check("pack with bad rows")
    finally:
        ar.free()


# ---- census, compact, expand -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("mult", [1, 2])
def test_census_compact_expand(ia, ctx, oracle, capfd, cus, mult, skew):
    """The census' tile size is traced; the compress kernel has the same 128-record tiles without a trace line, and the expand kernel
    stages two 128-element sub-tiles per tile (sort_compact.hpp), so mult = 2 — twice the tiles — gives IT the 3/4 shape."""
    tiny = ctx.alloc(24 * 16 + 16)
    tile, head = _probe(ctx, capfd, lambda: ctx.census(tiny.ptr + skew, 16))
    tiny.free()
    ntiles = mult * sw.choose_ntiles(cus)
    n = head + ntiles * tile + REST
    hist = sw.histogram(sw.sweep_plan(cus, 1, ntiles))
    assert max(hist) >= 4 and min(hist) >= 3, hist
    CHOSEN.append(f"sweep: census / compact (expand: half as many tiles): tile={tile} head={head} ntiles={ntiles} n={n} tiles per wave {dict(sorted(hist.items()))}")
    recs = oracle.generate(SEED + mult, 0, n, 16, 12)
    rng = np.random.default_rng(mult)
    rng.shuffle(recs)
    recs["index"] = rng.integers(0, 2**31, n, dtype=np.uint64)
    ar = _arena(ia, ctx, 24 * n, 12 * n, 24 * n)
    try:
        d, e, back = ar.carve(24 * n, skew), ar.carve(12 * n, 4 if skew else 0), ar.carve(24 * n, skew)
        d.upload(recs)
        got, rows = _traced(ctx, capfd, lambda: ctx.census(d, n))
        assert len(rows) == 1 and rows[0]["tiled"] == ntiles * tile and rows[0]["head"] == head and rows[0]["rest"] == REST, rows
        assert (got["or"], got["and"]) == kp.census_words(recs)
        assert got["order_drops"] and got["index_drops"]
        plan, want = ia.key_plan(got["or"], got["and"]), kp.Plan(got["or"], got["and"])
        assert plan.k == want.k <= 12
        ctx.compact(plan, d, n, e)
        ctx.expand(plan, e, n, back)
        ar.check("census / compact / expand")
        assert e.download(count=12 * n).tobytes() == kp.compact(want, recs).tobytes()
        assert back.download(count=24 * n).tobytes() == recs.tobytes()
        srt = recs[np.lexsort((recs["index"], recs["umi"], recs["barcode"]))]   # the flags on sorted input stay down over every tile seam
        d.upload(srt)
        got = ctx.census(d, n)
        assert not got["order_drops"] and (got["or"], got["and"]) == kp.census_words(srt)
    finally:
        ar.free()


# ---- the whitelist kernels -------------------------------------------------------------------------------------------
def _whitelist(ia, ctx, wl, bc_len):
    d = ctx.upload(np.ascontiguousarray(wl, dtype=np.uint64))
    try:
        return ia.Whitelist(ctx, d, len(wl), bc_len)
    finally:
        d.free()


def _counts(cls):
    k = np.bincount(cls, minlength=4)
    return {"exact": int(k[0]), "corrected": int(k[1]), "ambiguous": int(k[2]), "unmatched": int(k[3])}


def _chain_case(ia, ctx, capfd, rng, wl, bc, bc_len, skew, cls_skew, head, what, every_other=2000):
    """The chain of test_whitelist_chain on these barcodes, every result and every total against whitelist_np / resolve_np
    -> the traced rows of (correct, the masked add, resolve), one launch split each."""
    n = len(bc)
    recs = rnp.records(rng, bc)
    want, cls, counts = wnp.correct_records(recs, wl, bc_len, 1)
    first_tile = np.bincount(cls[head:head + 128], minlength=4)
    assert (first_tile > 0).all(), first_tile
    # the counters: exact and corrected reads of these records, then `every_other` reads of every other whitelist entry in a second
    # call, so that a pair of candidates is either lopsided (resolved) or even (below the share)
    extra = rnp.records(rng, wnp.with_junk(rng, np.repeat(np.unique(wl)[::2], every_other), bc_len))
    ab_np = rnp.add(rnp.add(rnp.Abundance(wl, bc_len), want, cls, 0b11), extra)
    out_np, cls_np, tot_np = rnp.resolve(ab_np, want, cls, 3, 4)
    assert tot_np["resolved"] > 0 and tot_np["below_share"] > 0 and tot_np["examined"] == counts["ambiguous"]
    ar = _arena(ia, ctx, 24 * n, n)
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
            d, d_cls = ar.carve(24 * n, skew), ar.carve(n, cls_skew)
            d.upload(recs)
            got_counts, rows_c = _traced(ctx, capfd, lambda: ctx.correct_barcodes(h, d, n, 1, d_cls))
            assert got_counts == counts == _counts(cls)
            assert (d_cls.download(np.uint8, n) == cls).all() and d.download(count=24 * n).tobytes() == want.tobytes()
            _, rows_a = _traced(ctx, capfd, lambda: ab.add(d, n, d_cls, 0b11))
            d_extra = ctx.upload(extra)
            ab.add(d_extra, len(extra))
            codes = np.concatenate([np.unique(wl), np.unique(wl)[:64] ^ np.uint64(1)])
            assert (ab.counts(codes) == rnp.counts(ab_np, codes)).all()
            tot, rows_r = _traced(ctx, capfd, lambda: ctx.resolve_barcodes(h, ab, d, n, d_cls, (3, 4)))
            d_extra.free()
            ar.check(what)
            assert tot == tot_np
            assert (d_cls.download(np.uint8, n) == cls_np).all() and d.download(count=24 * n).tobytes() == out_np.tobytes()
            assert len(rows_c) == len(rows_a) == len(rows_r) == 1
            return rows_c, rows_a, rows_r
    finally:
        ar.free()


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("kernel", ["correct_add", "resolve"])
def test_whitelist_chain(ia, ctx, capfd, cus, kernel, skew):
    """correct (class bytes, totals, records rewritten in place) -> Abundance.add under a class mask and again without one -> counts -> resolve, against
    whitelist_np / resolve_np.  A whitelist of 300 barcodes: every class occurs in every tile.  correct_add: sized by the 128-record
    tiles of ibu_k_correct and ibu_k_abundance_add, the 3/4 shape; resolve: sized by ibu_k_resolve's larger units, the 1/2 shape."""
    bc_len, w = 16, 300
    tiny, tiny_cls = ctx.upload(np.zeros(24 * 16 + 16, np.uint8)), ctx.upload(np.zeros(32, np.uint8))
    cls_skew = 15 if skew else 0                                 # ibu_k_resolve is split by its class bytes: one in front of a boundary
    with _whitelist(ia, ctx, np.arange(1, 9, dtype=np.uint64), bc_len) as h, h.abundance() as ab:
        probes = [_probe(ctx, capfd, lambda: ctx.correct_barcodes(h, tiny.ptr + skew, 16, 1, tiny_cls.ptr + cls_skew, counts=False)),
                  _probe(ctx, capfd, lambda: ab.add(tiny.ptr + skew, 16, tiny_cls.ptr + cls_skew, 1)),
                  _probe(ctx, capfd, lambda: ctx.resolve_barcodes(h, ab, tiny.ptr + skew, 16, tiny_cls.ptr + cls_skew, counts=False))]
    tiny.free()
    tiny_cls.free()
    assert probes[0] == probes[1] and probes[2][1] == probes[0][1]
    (tile, head), base = (probes[0], 3) if kernel == "correct_add" else (probes[2], 1)
    n, ntiles, plan = _shape("correct / abundance add" if kernel == "correct_add" else "resolve", cus, tile, head, base)
    rng = np.random.default_rng(0x1B00B00 + skew)
    wl, bc = rnp.make_case(rng, bc_len, w, n)
    rows_c, rows_a, rows_r = _chain_case(ia, ctx, capfd, rng, wl, bc, bc_len, skew, cls_skew, head, f"whitelist chain {kernel}")
    for r in (rows_c + rows_a if kernel == "correct_add" else rows_r):
        assert r["tiled"] == ntiles * tile and r["head"] == head and r["rest"] == REST, r


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("shape", ["waves", "workgroups"])
def test_whitelist_totals_of_waves_and_workgroups_without_a_tile(ia, ctx, capfd, cus, shape, skew):
    """The totals of correct and resolve come through a workgroup barrier (k_whitelist.hip: wl_flush_totals; kcommon.hpp:
    block_accumulate), so a wave that sweeps nothing must still reach it and a workgroup that sweeps nothing must add nothing.  The two shapes of tests/test_gpu_labels.py — waves: 61
    tiles, three waves of the last workgroup get none; workgroups: 4 cus + 1 tiles, where the CU count is a multiple of 8 the last
    workgroup gets none — each with a peeled head at skew 8 and a rest of 77 rows, so three launches add into one accumulator.  The
    same chain as above on a whitelist of 1000 barcodes.  Two per cent of one-base errors give no ambiguous record at 7 885 records
    (one planted pair among 1000 entries), so the barcodes are resolve_np.make_case's: 20 % one-base errors, 10 % midpoints of the
    planted pairs, 10 % random — resolve has work in every case, which the chain asserts on the numpy side."""
    bc_len, w, tile = 16, 1000, 128
    ntiles = 61 if shape == "waves" else 4 * cus + 1
    plan = sw.sweep_plan(cus, 1, ntiles)
    empty_workgroups = [b for b in range(len(plan) // 4) if not any(plan[4 * b:4 * b + 4])]
    if shape == "waves":
        assert len(plan) == 64 and [k for k, tiles in enumerate(plan) if not tiles] == [61, 62, 63] and not empty_workgroups
    else:
        assert len(plan) == 4 * cus and bool(empty_workgroups) == (cus % 8 == 0), (cus, empty_workgroups)
    head = 1 if skew else 0
    n = head + ntiles * tile + REST
    rng = np.random.default_rng([0x1B00B01, n, skew])
    wl, bc = rnp.make_case(rng, bc_len, w, n)
    rows_c, _, _ = _chain_case(ia, ctx, capfd, rng, wl, bc, bc_len, skew, 15 if skew else 0, head, f"whitelist totals {shape}", every_other=200)
    assert rows_c[0]["tiled"] == ntiles * tile and rows_c[0]["head"] == head and rows_c[0]["rest"] == REST, rows_c


# ---- the feature filter's class kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", SKEWS)
def test_filter_features(ia, ctx, capfd, cus, skew):
    from tests.test_gpu_features import _filter
    nf = 1000
    tiny, tiny_cls, tiny_cols = ctx.upload(np.zeros(24 * 16 + 16, np.uint8)), ctx.alloc(32), [ctx.upload(np.zeros(nf, np.uint64)) for _ in range(3)]
    tile, head = _probe(ctx, capfd, lambda: _filter(ia, ctx, ia.DeviceBuffer.wrap(ctx, tiny.ptr + skew, 24 * 16), 16, 1, nf, tiny_cols, fnp.limits(), tiny_cls, None))
    for t in [tiny, tiny_cls] + tiny_cols:
        t.free()
    n, ntiles, plan = _shape("filter_features", cus, tile, head)
    rng = np.random.default_rng(0x51500 + skew)
    recs = np.zeros(n, fnp.REC)
    w = recs.view(np.uint64).reshape(-1, 3)
    pal = np.concatenate([np.arange(nf, dtype=np.uint64), np.array([nf, nf + 1, 1 << 32, (1 << 32) + 5], np.uint64)])   # some out of range
    w[:, 0] = rng.integers(0, n // 20 + 2, n).astype(np.uint64)
    w[:, 1], w[:, 2] = pal[rng.integers(0, len(pal), n)], rng.integers(0, 50, n).astype(np.uint64)
    recs = recs[np.lexsort((w[:, 2], w[:, 1], w[:, 0]))]
    table, _ = fnp.feature_metrics(recs, nf, 1)
    q = lambda col, f: int(np.sort(col)[int(f * (nf - 1))])
    lim = fnp.limits(min_reads=max(q(table[0], 0.3), 1), max_reads=max(q(table[0], 0.9), 1), min_cells=2)
    v, cls, tot = fnp.filter_features(recs, nf, 1, table, lim)
    assert all(tot["reads_by_class"]) and all(tot["features_by_class"]), tot
    ar = _arena(ia, ctx, 24 * n, n, nf, 8 * nf, 8 * nf, 8 * nf)
    try:
        d, d_class, d_verdict = ar.carve(24 * n, skew), ar.carve(n, 3 if skew else 0), ar.carve(nf, 1)
        cols = [ar.carve(8 * nf, 0) for _ in range(3)]
        d.upload(recs)
        for col, t in zip(cols, table):
            col.upload(t)
        got, rows = _traced(ctx, capfd, lambda: _filter(ia, ctx, d, n, 1, nf, cols, lim, d_class, d_verdict))
        _assert_tiled(rows, n, ntiles, head)
        ar.check("filter_features")
        assert got == tot
        assert (d_verdict.download(np.uint8, nf) == v).all() and (d_class.download(np.uint8, n) == cls).all()
        assert d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
    finally:
        ar.free()


# ---- the unit loops (for u += nwaves, 2048 entries per unit) ---------------------------------------------------------
def _units(cus):
    """-> (n, plan): as many units as the 1/2 shape has tiles, the last one partial."""
    nunits = sw.choose_ntiles(cus, 1)
    plan = sw.sweep_plan(cus, 1, nunits)
    assert set(sw.histogram(plan)) == {1, 2}
    CHOSEN.append(f"sweep: unit loops: unit={UNIT} nunits={nunits} n={(nunits - 1) * UNIT + REST} units per wave {dict(sorted(sw.histogram(plan).items()))}")
    return (nunits - 1) * UNIT + REST, plan


@pytest.mark.parametrize("skew", SKEWS)
def test_select_records_over_two_units_per_wave(ia, ctx, cus, skew):
    """Class bytes that keep nothing in one whole unit and everything in the next, then a unit of mixed classes, and so on: a wave's
    second unit must start from its own count."""
    n, plan = _units(cus)
    rng = np.random.default_rng(0x5E1EC7 + skew)
    recs = np.zeros(n, wnp.REC)
    recs["barcode"], recs["umi"], recs["index"] = rng.integers(0, 1 << 62, n, dtype=np.uint64), rng.integers(0, 1 << 62, n, dtype=np.uint64), np.arange(n, dtype=np.uint64)
    unit = np.arange(n) // UNIT
    cls = np.where(unit % 3 == 0, 3, np.where(unit % 3 == 1, 0, rng.integers(0, 9, n))).astype(np.uint8)
    ar = _arena(ia, ctx, 24 * n, n, 24 * n)
    try:
        d, d_cls, d_out = ar.carve(24 * n, skew), ar.carve(n, 1 if skew else 0), ar.carve(24 * n, skew)
        d.upload(recs)
        d_cls.upload(cls)
        for keep in (0b0011, 0b1000, 0b0110):
            want = wnp.select(recs, cls, keep)
            k = C.c_size_t(0)
            ia._check(ia.lib.ibu_select_records(ctx._c, _p(d), _p(d_cls), n, keep, _p(d_out), n, C.byref(k), None))
            ar.check(f"select keep={keep:#b}")
            assert k.value == len(want) and 0 < len(want) < n
            assert d_out.download(count=24 * len(want)).tobytes() == want.tobytes(), keep
    finally:
        ar.free()


def test_matrix_rows_over_two_units_per_wave(ia, ctx, cus):
    from tests.test_gpu_mtx import _check_rows, _row_shape
    n, plan = _units(cus)
    _check_rows(ia, ctx, _row_shape("random", n), f"n={n} random")            # runs of 1 .. 8 entries: heads all over every unit
    _check_rows(ia, ctx, _row_shape("rows_2049", n), f"n={n} rows_2049")      # one head per unit, a row later in each


def test_matrix_market_body_over_two_units_per_wave(ia, ctx, cus):
    """A period of 11 lines whose numbers have 1 to 20 digits: 2048 is no multiple of 11, so every unit starts at another phase and
    the digit counts change inside every unit; the text is the period's text repeated."""
    n, plan = _units(cus)
    pattern = [0, 9, 10, 99, 100, 12345, (1 << 32) - 1, 1 << 32, 10**15, 10**19, (1 << 64) - 2]
    reps, rest = divmod(n, len(pattern))
    shifted = [pattern[3:] + pattern[:3], pattern[7:] + pattern[:7]]
    cols = [pattern, shifted[0], shifted[1]]
    block, block_max = mtx_np.body(*cols, 1, 1)
    tail, _ = mtx_np.body(*[c[:rest] for c in cols], 1, 1)
    want = block * reps + tail
    arrays = [np.tile(np.array(c, np.uint64), reps + 1)[:n] for c in cols]
    ar = _arena(ia, ctx, 8 * n, 8 * n, 8 * n, len(want))
    try:
        d_cols = [ar.carve(8 * n, 8 * (k & 1)) for k in range(3)]
        for d, a in zip(d_cols, arrays):
            d.upload(a)
        d_text = ar.carve(len(want), 3)
        nb, mx = C.c_size_t(0), (C.c_uint64 * 3)()
        ia._check(ia.lib.ibu_matrix_market_body(ctx._c, *[_p(c) for c in d_cols], n, 1, 1, _p(d_text), len(want), C.byref(nb), mx, None))
        ar.check("matrix market body")
        assert nb.value == len(want) and tuple(int(x) for x in mx) == block_max
        got = d_text.download(np.uint8, len(want))
        bad = np.flatnonzero(got != np.frombuffer(want, np.uint8))
        assert bad.size == 0, (int(bad[0]), bytes(got[max(int(bad[0]) - 20, 0):int(bad[0]) + 20]))
    finally:
        ar.free()
