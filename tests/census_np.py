"""Plain statement of the sort's census (ibu_amd/csrc/sort_census.hpp: OR / AND words, "some index is smaller than its predecessor's",
"some record is smaller than its predecessor") and the inputs of the seam tests: a base that is sorted AND in index order, the
single defects planted on it, and the rows at which the launcher's split of the rows (peeled head row | 128-record tiles | rest) and
the tiles themselves have their seams.  Test infrastructure — nothing in the product imports it."""
import numpy as np

from tests import keyplan_np as kp

REC = kp.REC
TILE = 128                                                    # records per census tile (kTileRecs)
WAVE = 64                                                     # rows per wave of the per-row (tail) kernel
U64 = np.uint64


def _fields(recs):
    recs = np.asarray(recs)
    assert recs.dtype == REC, recs.dtype
    return recs["barcode"], recs["umi"], recs["index"]        # uint64 columns: numpy compares them as unsigned


def drop_rows(recs):
    """(rows whose index is smaller than their predecessor's, rows whose record is smaller than their predecessor) — unsigned 64-bit
    comparisons, the record order lexicographic on (barcode, umi, index)."""
    b, u, x = _fields(recs)
    if len(b) < 2:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    pb, pu, px, b, u, x = b[:-1], u[:-1], x[:-1], b[1:], u[1:], x[1:]
    for col in (pb, pu, px, b, u, x):
        assert col.dtype == U64                               # (a mixed comparison would go through float64 and lose the low bits)
    less = (b < pb) | ((b == pb) & ((u < pu) | ((u == pu) & (x < px))))
    return np.flatnonzero(x < px) + 1, np.flatnonzero(less) + 1


def flags(recs):
    """(index_drops, order_drops) of a record array."""
    i, o = drop_rows(recs)
    return bool(len(i)), bool(len(o))


def words(recs):
    """(OR[3], AND[3]) of a record array."""
    return kp.census_words(recs)


# ---- where the seams are -------------------------------------------------------------------------------------------------------------
def split(n, peeled):
    """(head, main, rest): the peeled first row of an 8- but not 16-byte aligned array, the rows of whole tiles, the others."""
    head = 1 if peeled and n else 0
    main = ((n - head) // TILE) * TILE
    return head, main, n - head - main


IN_TILE = (1, 2, 63, 64, 65, 126, 127)                        # offsets inside a tile: lane L owns records 2L and 2L+1; lanes 0 and 63


def seam_candidates(n, peeled):
    """[(row, name, expressible)]: every seam row p the split of n rows names — the pair under test is (p - 1, p) — and whether that
    pair exists at this n."""
    head, main, rest = split(n, peeled)
    out = [(1, "row 1", n >= 2),
           (head, "peel/tile", head >= 1 and head < n)]
    out += [(head + TILE * k, f"tile seam {k}", TILE * k <= main and head + TILE * k < n) for k in (1, 2, 3)]
    out += [(head + main - TILE, "last tile", main >= TILE and head + main - TILE >= 1),
            (head + main, "main/rest", 1 <= head + main < n),
            (head + main + WAVE, "rest wave edge", rest > WAVE),
            (n - 1, "last row", n >= 2)]
    out += [(head + o, f"tile 0 + {o}", main >= TILE) for o in IN_TILE]
    return out


def seams(n, peeled):
    """[(row, names)] of the expressible seam rows of n rows, ascending, every row once."""
    rows = {}
    for p, name, ok in seam_candidates(n, peeled):
        if ok:
            assert 1 <= p < n, (n, peeled, p, name)
            rows.setdefault(p, []).append(name)
    return [(p, " = ".join(names)) for p, names in sorted(rows.items())]


def left_out(n, peeled):
    """Names of the seams that n rows cannot express (no such pair of rows)."""
    return [name for _, name, ok in seam_candidates(n, peeled) if not ok]


def tile_seams(n, peeled, tiles):
    """[(row, name)]: the first row of each of the given tiles (the seam towards the tile, or the peeled row, in front of it)."""
    head, main, _ = split(n, peeled)
    out = []
    for t in sorted(set(int(t) for t in tiles)):
        assert 0 <= t < main // TILE, (t, main // TILE)
        if head + TILE * t >= 1:
            out.append((head + TILE * t, f"tile {t}"))
    return out


def outlier_rows(n, peeled):
    """Rows for a lone OR / AND outlier: the seam rows, row 0, the last row (of a partly filled wave of the rest unless the rest is a
    multiple of 64) and the first rows of the waves — the records the kernels take as their reference."""
    head, main, rest = split(n, peeled)
    rows = dict(seams(n, peeled))
    extra = [(0, "row 0"), (n - 1, "last row"), (head, "first tiled row"), (head + main, "first row of the rest")]
    if rest > WAVE:
        extra.append((head + main + WAVE, "second wave of the rest"))
    for p, name in extra:
        if 0 <= p < n and p not in rows:
            rows[p] = name
    return sorted(rows.items())


# ---- the base and the defects -------------------------------------------------------------------------------------------------------
# Every record of the base has these bits set and the OUTLIER bits clear; all values stay below 2^62.
FIXED = {"barcode": (1 << 50) | (1 << 33), "umi": (1 << 52) | (1 << 33), "index": 1 << 36}
OUTLIER_SET = {"barcode": 61, "umi": 44, "index": 40}         # a bit no record of the base has
OUTLIER_CLEAR = {"barcode": 50, "umi": 52, "index": 36}       # a bit every record of the base has
RUN_MAX = 3                                                   # longest run of one barcode in the base


def clean_base(n, seed):
    """n records that are sorted and in index order: barcodes non-decreasing in runs of 1 .. 3, umis non-decreasing inside a barcode
    with ties, index = 4 * row.  Distinct barcodes and distinct umis of a barcode are 8 apart, so that a defect has room."""
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=REC)
    if n == 0:
        return recs
    starts = np.concatenate(([0], np.cumsum(rng.integers(1, RUN_MAX + 1, n))))
    new_run = np.zeros(n, dtype=bool)
    new_run[starts[starts < n]] = True
    run_id = np.cumsum(new_run)                               # 1, 1, 2, 3, 3, 3, ...
    step = np.where(new_run, 0, rng.integers(0, 2, n))        # umi: stays or rises inside a run
    pos = np.arange(n)
    run_start = np.maximum.accumulate(np.where(new_run, pos, 0))
    csum = np.cumsum(step)
    umi_in_run = csum - csum[run_start]
    recs["barcode"] = (U64(FIXED["barcode"]) | (run_id.astype(U64) * U64(8)))
    recs["umi"] = U64(FIXED["umi"]) | ((umi_in_run.astype(U64) + U64(1 + seed % 5)) * U64(8))
    recs["index"] = U64(FIXED["index"]) | (pos.astype(U64) * U64(4))
    assert 8 * (n + 1) < 1 << 32 and 4 * n < 1 << 32          # the low parts stay below the fixed bits
    return recs


KINDS = ("1", "2", "3", "4", "5", "6", "1h", "3h", "4h", "1s", "3s", "4s")
HI = 1 << 33                                                  # set in every barcode and umi of the base: a fall in the high 32 bits
TOP = 1 << 63


def plant(base, p, kind):
    """{row: (barcode, umi, index)}: the one to three records that plant ONE defect of the given kind on the pair (p - 1, p) of a
    clean base; A = base[p - 1], B = base[p].
      1   index falls, barcode and umi equal              2   index falls, barcode rises
      3   barcode falls, index rises                      4   umi falls inside an equal barcode, index rises
      5   barcode rises, umi falls                        6   B is an exact copy of A
      1h / 3h / 4h   as 1 / 3 / 4 with the fall in the high 32 bits only, the low 32 bits rise
      1s / 3s / 4s   as 1 / 3 / 4 with the two values on either side of 2^63"""
    n = len(base)
    assert 1 <= p < n

    def rec(i):
        return [int(base["barcode"][i]), int(base["umi"][i]), int(base["index"][i])]

    a, b = rec(p - 1), rec(p)
    out = {}

    def raise_barcode_from_p():                               # B (and what follows it in A's run) gets a barcode of its own, A's + 1
        if b[0] != a[0]:
            return
        i = p
        while i < n and int(base["barcode"][i]) == a[0]:
            r = out.get(i) or rec(i)
            r[0] = a[0] + 1
            out[i] = r
            i += 1

    if kind == "1":
        out[p] = [a[0], a[1], a[2] - 1]
    elif kind == "2":
        out[p - 1] = [a[0], a[1], a[2] + 2]
        out[p] = [b[0], b[1], a[2] + 1]
        raise_barcode_from_p()
    elif kind == "3":
        out[p] = [a[0] - 1, b[1], b[2]]
    elif kind == "4":
        out[p] = [a[0], a[1] - 1, b[2]]
    elif kind == "5":
        out[p] = list(b)
        raise_barcode_from_p()
        out[p - 1] = [a[0], max(a[1], out[p][1] + 1), a[2]]   # A ends its run now: a larger umi there disturbs nothing behind it
    elif kind == "6":
        out[p] = list(a)
    elif kind == "1h":
        out[p - 1] = [a[0], a[1], a[2] + (1 << 32)]
        out[p] = [a[0], a[1], a[2] + 1]
    elif kind == "3h":
        out[p] = [a[0] - HI + 1, b[1], b[2]]
    elif kind == "4h":
        out[p] = [a[0], a[1] - HI + 1, b[2]]
    elif kind == "1s":
        out[p - 1] = [a[0], a[1], a[2] | TOP]
        out[p] = [a[0], a[1], a[2] + 1]
    elif kind == "3s":
        out[p - 1] = [a[0] | TOP, a[1], a[2]]
    elif kind == "4s":
        out[p - 1] = [a[0], a[1] | TOP, a[2]]
        out[p] = [a[0], a[1], b[2]]
    else:
        raise ValueError(kind)
    assert 1 <= len(out) <= 3 and max(out) - min(out) <= 2, (p, kind, sorted(out))
    return {i: tuple(r) for i, r in out.items()}


# what each kind must do to the flags (index_drops, order_drops): the pair (p - 1, p) and no other
KIND_FLAGS = {"1": (True, True), "2": (True, False), "3": (False, True), "4": (False, True), "5": (False, False), "6": (False, False),
              "1h": (True, True), "3h": (False, True), "4h": (False, True), "1s": (True, True), "3s": (False, True), "4s": (False, True)}


def plant_bit(base, row, field, clear):
    """{row: record}: one record with the field's outlier bit set (a bit no other record has) or its fixed bit cleared."""
    r = {f: int(base[f][row]) for f in kp.FIELDS}
    if clear:
        assert r[field] >> OUTLIER_CLEAR[field] & 1
        r[field] &= ~(1 << OUTLIER_CLEAR[field])
    else:
        assert not r[field] >> OUTLIER_SET[field] & 1
        r[field] |= 1 << OUTLIER_SET[field]
    return {row: (r["barcode"], r["umi"], r["index"])}


def apply(recs, patch):
    """A copy of recs with the patch's records written."""
    out = recs.copy()
    for i, r in patch.items():
        out[i] = r
    return out


class Base:
    """A record array whose own flags are (False, False), with what a patch of a few neighbouring rows makes of the statement —
    without another pass over all n records: a pair that the patch does not touch is a pair of the base and adds no flag, and the
    words are those of the untouched rows in front of the patch, of the patched rows and of the untouched rows behind it."""

    def __init__(self, recs):
        self.recs = recs
        self.n = n = len(recs)
        assert flags(recs) == (False, False)
        self._pre_or, self._pre_and, self._suf_or, self._suf_and = [], [], [], []
        for f in kp.FIELDS:
            col = recs[f]
            self._pre_or.append(np.concatenate(([U64(0)], np.bitwise_or.accumulate(col))))          # [i]: rows [0, i)
            self._pre_and.append(np.concatenate(([~U64(0)], np.bitwise_and.accumulate(col))))
            self._suf_or.append(np.concatenate((np.bitwise_or.accumulate(col[::-1])[::-1], [U64(0)])))   # [i]: rows [i, n)
            self._suf_and.append(np.concatenate((np.bitwise_and.accumulate(col[::-1])[::-1], [~U64(0)])))
        assert n == 0 or words(recs) == ([int(w[n]) for w in self._pre_or], [int(w[n]) for w in self._pre_and])

    def window(self, patch):
        """(lo, patched rows [lo, hi)): the patch's rows with one untouched neighbour on either side."""
        lo, hi = max(min(patch) - 1, 0), min(max(patch) + 2, self.n)
        return lo, apply(self.recs[lo:hi], {i - lo: r for i, r in patch.items()})

    def expect(self, patch):
        """{"index_drops", "order_drops", "or", "and"} of the base with the patch applied."""
        lo, win = self.window(patch)
        hi = lo + len(win)
        idx, order = flags(win)
        w_or, w_and = words(win)
        return {"index_drops": idx, "order_drops": order,
                "or": [int(self._pre_or[f][lo]) | w_or[f] | int(self._suf_or[f][hi]) for f in range(3)],
                "and": [int(self._pre_and[f][lo]) & w_and[f] & int(self._suf_and[f][hi]) for f in range(3)]}


# the sizes of the seam tests: the per-row kernel alone; exactly one tile; one tile with the head row and the rest on either side;
# 128 + 5, kept for coverage only: a rest of at most 64 rows leaves the second wave of the per-row kernel without rows, but such a
# wave takes recs[row0] for its reference, a row of the launch, so nothing it could add shows; three tiles and a rest with and
# without the head row; and one at which a wave of a full grid walks three tiles
SMALL_SIZES = (2, 3, 64, 65, 127, 128, 129, 130, 128 + 5, 257, 3 * 128 + 37, 1 + 3 * 128 + 37)
LARGE_SIZE = 2_000_003
