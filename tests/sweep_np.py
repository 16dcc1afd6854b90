"""The persistent sweep of the tiled kernels, stated in Python: which tiles every wave of a launch visits, in which order.

A mirror of the launch plan in ibu_amd/csrc (kcommon.hpp: grid_for, logical_block, tile_range; kernels.h: resident_blocks' cap) for
the default build: IBU_BLOCK = 256 (four waves per workgroup), IBU_XCD_REMAP = 1, IBU_XCD_STATIC = 1, IBU_XCD_SUB = 1.  Workgroup i
runs on XCD i % 8.  A grid that is a multiple of 8 gives every XCD one fixed eighth of the tiles (`tpp = ceil(ntiles / 8)`, the last
part is what is left), swept by the XCD's waves with a stride of that many waves; any other grid falls back to the identity order
with a stride of all waves.  The tests use it to CHOOSE sizes at which every wave iterates (tests/test_gpu_sweeps.py) and to name
the tiles of one wave; the device side is checked there, because a tile visited twice or not at all shows in the outputs."""
from collections import Counter

WAVES_PER_BLOCK = 4            # kWavesPerBlock
XCDS = 8
EXTRA = 38                     # waves of an XCD that get one tile more than the others in the chosen shapes


def grid_for(ntiles, cus, blocks_per_cu):
    """kcommon.hpp grid_for with resident_blocks' cap: every tiled kernel fits at least `blocks_per_cu = 1` workgroup per CU, so at
    that setting the cap is `cus` whatever the kernel's occupancy is."""
    need = (ntiles + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK
    cap = cus * blocks_per_cu
    return max(need, 1) if need < cap else cap


def logical_block(block, grid):
    """kcommon.hpp logical_block: XCD x gets the x-th eighth of the logical order; grids that are no multiple of 8: identity."""
    if grid & 7:
        return block
    return (block & 7) * (grid >> 3) + (block >> 3)


def tile_range(grid, block, wib, ntiles):
    """kcommon.hpp tile_range -> (first tile, stride, end) of wave `wib` of workgroup `block`."""
    if grid % XCDS == 0 and grid >= XCDS:
        tpp = (ntiles + XCDS - 1) // XCDS
        xcd, lb, nbx = block & 7, block >> 3, grid >> 3
        t0 = xcd * tpp
        t1 = min(t0 + tpp, ntiles)
        return t0 + lb * WAVES_PER_BLOCK + wib, nbx * WAVES_PER_BLOCK, (t1 if t0 < ntiles else 0)
    return logical_block(block, grid) * WAVES_PER_BLOCK + wib, grid * WAVES_PER_BLOCK, ntiles


def grid_plan(grid, ntiles):
    """The tiles of every wave of a grid of `grid` workgroups, in sweep order; wave 4 b + w is wave w of workgroup b."""
    plan = []
    for block in range(grid):
        for wib in range(WAVES_PER_BLOCK):
            t, stride, end = tile_range(grid, block, wib, ntiles)
            plan.append(list(range(t, end, stride)))
    return plan


def sweep_plan(cus, blocks_per_cu, ntiles):
    """The plan of a tiled kernel's launch over `ntiles` tiles on a device of `cus` CUs."""
    return grid_plan(grid_for(ntiles, cus, blocks_per_cu), ntiles)


def histogram(plan):
    """{tiles per wave: number of waves}."""
    return dict(Counter(len(w) for w in plan))


def _extra(waves):
    # One tile more for EXTRA waves of the `waves` that share a range.  The rest must exist for the histogram to have two classes, so
    # a device with no more than EXTRA such waves (fewer than 80 CUs: none of the parts this library runs on) gives half of them one,
    # and at least the three that the short last part takes back.
    return EXTRA if waves > EXTRA else max(waves // 2, 3)


def choose_ntiles(cus, base=3):
    """ntiles at blocks_per_cu = 1 such that every wave sweeps `base` or `base + 1` tiles (base = 3: the sweep returns to register
    set `a` with data prefetched during phase B, and ends in phase A for some waves and in phase B for others; base = 1: the
    smaller shape for expensive references).  cus % 8 == 0: `wpx = cus / 8 * 4` waves per XCD, `tpp = base * wpx + 38` tiles per
    part and `ntiles = 8 tpp - 3`, so the last XCD's part is three tiles short; 256 CUs at base 3 give 3373.  Any other `cus`: the
    stride form, `base * 4 cus + 37`."""
    if cus % XCDS == 0:
        wpx = cus // XCDS * WAVES_PER_BLOCK
        tpp = base * wpx + _extra(wpx)
        ntiles = XCDS * tpp - 3
    else:
        waves = cus * WAVES_PER_BLOCK
        ntiles = base * waves + (EXTRA - 1 if waves >= EXTRA else _extra(waves))
    assert grid_for(ntiles, cus, 1) == cus, "the grid must sit at its cap"
    return ntiles


def wave_with(plan, count, last_tile=None):
    """The first wave that sweeps `count` tiles (and, if given, ends on `last_tile`)."""
    for w in plan:
        if len(w) == count and (last_tile is None or w[-1] == last_tile):
            return w
    raise LookupError(f"no wave with {count} tiles" + ("" if last_tile is None else f" ending on tile {last_tile}"))


def owner(plan, tile):
    """The wave that visits `tile`."""
    for w in plan:
        if tile in w:
            return w
    raise LookupError(f"tile {tile} is in no wave's sweep")
