"""tests/sweep_np.py, the Python statement of the tiled kernels' launch plan: the waves' tiles partition [0, ntiles) for every grid
the launchers can choose, and the sizes tests/test_gpu_sweeps.py takes from it make every wave iterate as that file says."""
import pytest

from tests import sweep_np as sw

GRIDS = range(1, 4 * 256 + 1)
NTILES = sorted({*range(0, 301), *range(0, 5001, 97), 5000,
                 *(m + d for m in range(0, 5001, 1024) for d in range(-9, 10) if 0 <= m + d <= 5000)})


DENSE_GRIDS = {*range(1, 17), 24, 32, 33, 64, 256, 304}      # these meet every value of NTILES; the others one each, in rotation


def test_every_tile_is_swept_exactly_once():
    assert all(t in NTILES for t in (0, 1, 300, 1015, 1024, 1033, 4087, 4105, 5000))
    met = set()
    for grid in GRIDS:
        nwaves = grid * sw.WAVES_PER_BLOCK
        some = NTILES if grid in DENSE_GRIDS else [NTILES[(5 * grid) % len(NTILES)]]
        met.update(some)
        for ntiles in some:
            seen = bytearray(ntiles)
            for block in range(grid):
                for wib in range(sw.WAVES_PER_BLOCK):
                    t, stride, end = sw.tile_range(grid, block, wib, ntiles)
                    assert end <= ntiles and 0 < stride <= nwaves
                    for tile in range(t, end, stride):
                        assert not seen[tile], (grid, ntiles, tile)
                        seen[tile] = 1
            assert all(seen), (grid, ntiles, seen.index(0))
    assert met == set(NTILES)


def test_grid_plan_is_the_tile_ranges_in_wave_order():
    plan = sw.grid_plan(16, 203)              # tpp = 26: XCD 7 holds tiles 182 .. 202
    assert len(plan) == 64
    assert plan[0] == [0, 8, 16, 24] and plan[3] == [3, 11, 19]
    assert plan[4] == [26, 34, 42, 50]        # workgroup 1 runs on XCD 1
    assert plan[4 * 8] == [4, 12, 20]         # workgroup 8: the second workgroup of XCD 0
    assert plan[4 * 15 + 3] == [189, 197]     # the short last part
    assert sw.grid_plan(3, 30)[5] == [5, 17, 29]   # not a multiple of 8: identity order, stride of all waves
    assert sw.grid_plan(8, 3) == [[0], [], [], [], [1], [], [], [], [2]] + [[]] * 23   # parts past the end are empty


@pytest.mark.parametrize("ntiles,cus,bpc,want", [(0, 256, 7, 1), (1, 256, 7, 1), (4, 256, 7, 1), (5, 256, 7, 2), (7167, 256, 7, 1792),
                                                 (7168, 256, 7, 1792), (10**6, 256, 7, 1792), (1023, 256, 1, 256), (3373, 256, 1, 256)])
def test_grid_for(ntiles, cus, bpc, want):
    assert sw.grid_for(ntiles, cus, bpc) == want


def test_below_the_cap_no_wave_iterates():
    """What the issue behind tests/test_gpu_sweeps.py rests on: until the grid reaches its cap every wave has at most one tile."""
    for ntiles in NTILES:
        if sw.grid_for(ntiles, 256, 7) < 256 * 7:
            assert max(map(len, sw.sweep_plan(256, 7, ntiles)), default=0) <= 1, ntiles


@pytest.mark.parametrize("cus", [8, 64, 256, 304])
def test_the_chosen_shapes(cus):
    wpx = cus // 8 * 4
    extra = 38 if wpx > 38 else max(wpx // 2, 3)
    for base in (3, 1):
        ntiles = sw.choose_ntiles(cus, base)
        plan = sw.sweep_plan(cus, 1, ntiles)
        assert len(plan) == 4 * cus and sorted(t for w in plan for t in w) == list(range(ntiles))
        # XCDs 0 .. 6: `extra` waves with one tile more; the last XCD's part is three tiles shorter
        assert sw.histogram(plan) == {base + 1: 8 * extra - 3, base: 8 * (wpx - extra) + 3}
        tpp = (ntiles + 7) // 8
        assert ntiles == 8 * tpp - 3
        last = [w for w in plan if w and w[0] >= 7 * tpp]
        assert sum(map(len, last)) == tpp - 3 and sw.histogram(last) == {k: v for k, v in ((base + 1, extra - 3), (base, wpx - extra + 3)) if v}
        assert sw.owner(plan, ntiles - 1) in last
        # sweeps of base + 1 = 4 tiles end in phase B, those of 3 in phase A
        assert len(sw.wave_with(plan, base + 1)) == base + 1
    if cus == 256:
        assert sw.choose_ntiles(256) == 3373 and sw.choose_ntiles(256, 1) == 8 * (128 + 38) - 3
        assert sw.histogram(sw.sweep_plan(256, 1, 3373)) == {4: 8 * 38 - 3, 3: 8 * 90 + 3}
    if cus == 304:
        assert sw.choose_ntiles(304) == 8 * (3 * 152 + 38) - 3


@pytest.mark.parametrize("cus", [10, 100, 228])
def test_the_chosen_shapes_without_xcd_parts(cus):
    """cus % 8 != 0: the grid at its cap is no multiple of 8 and the stride form applies."""
    for base in (3, 1):
        ntiles = sw.choose_ntiles(cus, base)
        assert ntiles == base * 4 * cus + 37
        plan = sw.sweep_plan(cus, 1, ntiles)
        assert sorted(t for w in plan for t in w) == list(range(ntiles))
        assert sw.histogram(plan) == {base + 1: 37, base: 4 * cus - 37}
