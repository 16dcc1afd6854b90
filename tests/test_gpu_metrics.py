"""Per-barcode QC metrics and the barcode filter on the device (ibu_barcode_metrics, ibu_filter_barcodes): every comparison is byte
for byte against the numpy statement of the semantics in tests/metrics_np.py, the twelve totals included; every call goes through
the C ABI, and every buffer — the columns at exactly 8 B per barcode, d_class at exactly n bytes, the bitmap at its words — is
carved at its contract size out of an arena with guard zones (the pattern of tests/test_gpu_cells.py).  The records are compared
after every case: they are never written."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest

from tests import count_np
from tests import metrics_np as mnp
from tests.test_gpu_count import PATTERN, _arena, _p

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 127, 128, 129, 255, 2559, 2561, 100_003]
SEG, TILE = 8192, 128                                            # runs_walk.hpp: records per segment / per tile
SEAM_ROWS = [(SEG * k, d) for k in (1, 2, 12) for d in (-1, 0, 1)] + [(TILE * k, d) for k in (3, 63, 65) for d in (-1, 0, 1)]
BIG = 1_000_003
NS = SIZES + [s + d for s, d in SEAM_ROWS]
SKEWS = [0, 8]                                                   # 16-byte aligned / 8- but not 16-byte aligned base
SHAPES = ["own_barcode", "one_barcode", "seam", "span", "random"]
GRID = [(n, skew, shape) for n, skew, shape in itertools.product(NS, SKEWS, SHAPES) if shape != "span" or n > 4 * SEG]
GRID += [(BIG, 0, "own_barcode"), (BIG, 8, "random")]            # one size of 1e6, for two shapes only
assert len(set(NS)) == len(NS) == 29 and len(GRID) == 2 * (29 * 4 + 4) + 2, len(GRID)
GARBAGE = 0x5A5A5A5A5A5A5A5A
# the values the second and third words take: around the set sizes 1, 64 and 65 (a value equal to set_bits is in the data), around
# the bitmap's word boundary, and above 2^32 (its low bits, 7, are the number of a set bit)
PALETTE = np.array([0, 1, 7, 63, 64, 65, 62, (1 << 32) + 7], np.uint64)
# (bits that are set, set_bits): none; one bit; 64 and 65 bits with the top bit set
SETS = [(None, 0), ([0], 1), ([1, 7, 63], 64), ([0, 7, 62, 64], 65)]


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _metrics(ia, ctx, d, n, d_set, bits, word, cols, cap, stream=None):
    """One ibu_barcode_metrics call through the C ABI -> *n_barcodes; cols = six DeviceBuffers or None."""
    nb = C.c_size_t(12345)
    ia._check(ia.lib.ibu_barcode_metrics(ctx._c, _p(d), n, _p(d_set), bits, word, *[_p(c) for c in cols], cap, C.byref(nb), stream))
    return nb.value


def _garbage_counts():
    from ibu_amd import _lib
    four = lambda: (C.c_uint64 * 4)(*[GARBAGE] * 4)
    return _lib.CBarcodeFilterCounts(GARBAGE, four(), four(), GARBAGE, GARBAGE, GARBAGE)


def _filter(ia, ctx, d, n, d_set, bits, word, lim, d_class, want_counts=True, stream=None):
    """One ibu_filter_barcodes call through the C ABI -> the totals as metrics_np states them (None without counts)."""
    from ibu_amd import _lib
    c = _garbage_counts()
    l = _lib.CBarcodeLimits(*[lim[f] for f in mnp.LIMITS])
    ia._check(ia.lib.ibu_filter_barcodes(ctx._c, _p(d), n, _p(d_set), bits, word, C.byref(l), _p(d_class), C.byref(c) if want_counts else None, stream))
    if not want_counts:
        return None
    return {"barcodes": int(c.barcodes), "barcodes_by_class": tuple(int(x) for x in c.barcodes_by_class),
            "reads_by_class": tuple(int(x) for x in c.reads_by_class), "triples_passed": int(c.triples_passed),
            "set_triples_passed": int(c.set_triples_passed), "reserved": int(c.reserved)}


def _base(n):
    """Barcodes of three records: two or three pairs, three triples."""
    r = np.zeros(n, mnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.int64)
    w[:, 0] = (i // 3).astype(np.uint64)
    w[:, 1] = PALETTE[(i // 3 + (i % 3) // 2) % 8]
    w[:, 2] = PALETTE[i % 8]
    return r, w


def _seam(n, head, d):
    """At every seam row s + d + head that fits, a barcode A of ten records (five pairs, ten triples, second words 0 1 7 62 63) ends
    just in front of the row and a barcode B of two records begins on it.  At every other seam B's first record repeats the second
    and third word of A's last, so that the barcode head is no change of the lower levels' words; at the others all three words
    change.  A's records are mostly in the 64- and 65-bit sets, B's second never: the two differ in their share, and under
    min_pairs = 3 in their class."""
    r, w = _base(n)
    laid = []
    for k, s in enumerate(sorted({s for s, _ in SEAM_ROWS})):
        row = s + d + head
        big = (1 << 40) + 2 * k
        if row - 10 < 0 or row + 2 > n:
            continue
        w[row - 10:row, 0] = big
        w[row - 10:row, 1] = np.repeat(np.array([0, 1, 7, 62, 63], np.uint64), 2)
        w[row - 10:row, 2] = np.tile(np.array([7, 63], np.uint64), 5)
        w[row:row + 2, 0] = big + 1
        w[row:row + 2, 1] = [63, 64] if k & 1 else [64, 65]
        w[row:row + 2, 2] = [63, 64] if k & 1 else [65, (1 << 32) + 7]
        laid.append(row)
    return r, laid


def _span(n, head):
    """One barcode from just in front of the second segment to just behind the fourth, its pairs 1000 records and its triples 7."""
    r, w = _base(n)
    a, b = head + SEG - 6, head + 4 * SEG + 9
    a, b = a - (a % 3), b - (b % 3)
    j = np.arange(b - a)
    w[a:b, 0], w[a:b, 1], w[a:b, 2] = 1 << 41, PALETTE[(j // 1000) % 8], PALETTE[(j // 7) % 8]
    return r


def _random(n):
    """About 100 large barcodes among small ones; inside a barcode the second word changes every a records, the third every b."""
    rng = np.random.default_rng(0x41300 + n)
    large = min(100, n // 600 + 1)
    lens = []
    total = 0
    while total < n:
        lens += rng.integers(1, 4, 40).tolist() + [int(rng.integers(n // (3 * large) + 1, n // (2 * large) + 2))]
        total = sum(lens)
    lens = np.array(lens, np.int64)
    first = np.repeat(np.cumsum(lens) - lens, lens)[:n]
    which = np.repeat(np.arange(len(lens)), lens)[:n]
    a, b = rng.integers(1, 6, len(lens))[which], rng.integers(1, 4, len(lens))[which]
    j = np.arange(n) - first
    r = np.zeros(n, mnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    w[:, 0], w[:, 1], w[:, 2] = (which * 3 + 11).astype(np.uint64), PALETTE[(j // (a * b)) % 8], PALETTE[(j // b + which) % 8]
    return r


@functools.lru_cache(maxsize=4)
def _shape(shape, n, skew, d=0):
    r = np.zeros(n, mnp.REC)
    w = r.view(np.uint64).reshape(-1, 3)
    i = np.arange(n, dtype=np.int64)
    if shape == "own_barcode":
        w[:, 0], w[:, 1], w[:, 2] = i.astype(np.uint64), PALETTE[i % 8], PALETTE[(i // 3) % 8]
    elif shape == "one_barcode":
        w[:, 0], w[:, 1], w[:, 2] = 5, PALETTE[(i >> 2) % 8], PALETTE[(i >> 1) % 8]
    elif shape == "seam":
        r = _seam(n, min(skew // 8, n), d)[0]
    elif shape == "span":
        r = _span(n, min(skew // 8, n))
    else:
        r = _random(n)
    assert len(r) == n
    return r


def _equality_limits(table, set_of):
    """Limits under which the first barcode with a share strictly between 0 and 1 sits exactly on the bound (None: there is none)."""
    x, set_x = (table[3], table[5]) if set_of else (table[1], table[4])
    for k in np.flatnonzero((set_x > 0) & (set_x < x))[:1]:
        g = math.gcd(int(set_x[k]), int(x[k]))
        if int(x[k]) // g < 1 << 24:
            return mnp.limits(set_num=int(set_x[k]) // g, set_den=int(x[k]) // g, set_of=set_of), int(k)
    return None


def _limit_sets(table, word):
    """The limits a case is filtered with: nothing, one that reaches LOW, HIGH and SET from the table's own quantiles, and the
    equality case."""
    reads, pairs, triples = table[1], table[2], table[3]
    q = lambda c, f: int(np.sort(c)[int(f * (len(c) - 1))])
    out = [mnp.limits(),
           mnp.limits(min_pairs=3, set_num=1, set_den=3, set_of=word - 1),
           mnp.limits(min_reads=q(reads, 0.2), max_pairs=max(q(pairs, 0.8), 1), min_triples=q(triples, 0.1), max_triples=max(q(triples, 0.9), 1),
                      max_reads=max(q(reads, 0.95), 1), set_num=2, set_den=5, set_of=2 - word)]
    eq = _equality_limits(table, word - 1)
    if eq:
        out.append(eq[0])
    return out


def _check_case(ia, ctx, recs, n, skew, full=True):
    """Every set and both set words: the table at its exact capacity, the filter under several limits, into d_class at exactly n
    bytes.  full: also the size query, a capacity of one less, every column NULL in turn and the totals-only call."""
    B = int(1 + np.count_nonzero(recs["barcode"][1:] != recs["barcode"][:-1])) if n else 0
    ar = _arena(ia, ctx, 24 * n, n, n, *[8 * B] * 6, *[16] * len(SETS))
    try:
        d = ar.carve(24 * n, skew)
        d_classes = [ar.carve(n, 0), ar.carve(n, 3)]              # (with the one record a skewed base peels: word and byte stores of the fill)
        cols = [ar.carve(8 * B, 8 * (j & 1)) for j in range(6)]
        d_sets = []
        for values, bits in SETS:
            words = mnp.bitmap(values or [], bits)
            d_sets.append(ar.carve(8 * len(words), 8) if bits else None)
            if bits:
                d_sets[-1].upload(words)
        if n:
            d.upload(recs)
        reached = set()
        for (j, (values, bits)), word in itertools.product(enumerate(SETS), (1, 2)):
            words, d_set = mnp.bitmap(values or [], bits), d_sets[j]
            what = f"set of {bits} bits, word {word}"
            table = mnp.barcode_metrics(recs, words, bits, word)
            assert len(table[0]) == B
            assert _metrics(ia, ctx, d, n, d_set, bits, word, cols, B) == B, what
            ctx.synchronize()
            for name, col, want in zip(mnp.COLUMNS, cols, table):
                have = col.download(np.uint64, B) if B else np.empty(0, np.uint64)
                bad = np.flatnonzero(have != want)
                assert bad.size == 0, f"{what}: {name} differs in {bad.size} rows, first at {int(bad[0])}: {int(have[bad[0]])} for {int(want[bad[0]])}"
            if full and (j, word) in ((2, 1), (3, 2)):
                assert _metrics(ia, ctx, d, n, d_set, bits, word, [None] * 6, 0) == B, "the size query"
                if B:
                    before = [c.download(np.uint64, B).tobytes() for c in cols]
                    nb = C.c_size_t(12345)
                    with pytest.raises(ia.IbuError) as ei:
                        ia._check(ia.lib.ibu_barcode_metrics(ctx._c, _p(d), n, _p(d_set), bits, word, *[_p(c) for c in cols], B - 1, C.byref(nb), None))
                    assert ei.value.kind == "InvalidArg" and nb.value == B and (ei.value.a, ei.value.b) == (B, B - 1)
                    ctx.synchronize()
                    assert [c.download(np.uint64, B).tobytes() for c in cols] == before, "a capacity of one less: nothing is written"
                    for skip in range(6):                         # every column NULL in turn: the others are written, this one is not
                        for c in cols:
                            c.upload(np.full(8 * B, PATTERN, np.uint8))
                        given = [None if k == skip else c for k, c in enumerate(cols)]
                        assert _metrics(ia, ctx, d, n, d_set, bits, word, given, B) == B
                        ctx.synchronize()
                        for k, (c, want) in enumerate(zip(cols, table)):
                            have = c.download(np.uint64, B).tobytes()
                            assert have == (np.full(8 * B, PATTERN, np.uint8).tobytes() if k == skip else want.tobytes()), (what, skip, k)
                ar.check(what + ", the forms of the metrics call")
            for i, lim in enumerate(_limit_sets(table, word) if n else [mnp.limits(), mnp.limits(min_pairs=3, set_num=1, set_den=3)]):
                d_class = d_classes[(i + j) & 1]
                cls, tot = mnp.filter_barcodes(recs, words, bits, word, lim, table)
                got = _filter(ia, ctx, d, n, d_set, bits, word, lim, d_class)
                assert got == tot, (what, lim, got, tot)
                reached |= {c for c in range(4) if tot["barcodes_by_class"][c]}
                if n:
                    have = d_class.download(np.uint8, n)
                    bad = np.flatnonzero(have != cls)
                    assert bad.size == 0, f"{what} {lim}: {bad.size} class bytes differ, first at row {int(bad[0])}: {int(have[bad[0]])} for {int(cls[bad[0]])}"
                if full and i == 1:
                    assert _filter(ia, ctx, d, n, d_set, bits, word, lim, None) == tot, "totals only"
            if full or j == 0:
                ar.check(what)
        ar.check("metrics")
        assert n == 0 or d.download(count=24 * n).tobytes() == recs.tobytes(), "the records are read only"
        return reached
    finally:
        ar.free()


@pytest.mark.parametrize("n,skew,shape", GRID)
def test_metrics_and_filter_match_numpy(ia, ctx, n, skew, shape):
    for d in ((-1, 0, 1) if shape == "seam" and n > TILE * 3 else (0,)):
        reached = _check_case(ia, ctx, _shape(shape, n, skew, d), n, skew, full=n < BIG)
        if shape in ("seam", "random") and n >= 2559:
            assert reached == {0, 1, 2, 3}, reached


def test_the_shapes_have_what_they_claim():
    for d in (-1, 0, 1):
        recs, laid = _seam(100_003, 0, d)
        assert laid == [s + d for s in sorted({s for s, _ in SEAM_ROWS})], (d, laid)
        w = recs.view(np.uint64).reshape(-1, 3)
        same = [bool((w[row, 1:] == w[row - 1, 1:]).all()) for row in laid]
        assert same == [bool(k & 1) for k in range(len(laid))], "the lower words change at every other seam only"
        assert all(w[row, 0] != w[row - 1, 0] and w[row - 10, 0] != w[row - 11, 0] for row in laid)
        words = mnp.bitmap(*SETS[2])
        table = mnp.barcode_metrics(recs, words, 64, 1)
        cls = mnp.filter_barcodes(recs, words, 64, 1, mnp.limits(min_pairs=3), table)[0]
        assert all(cls[row - 1] == mnp.PASS and cls[row] == mnp.LOW for row in laid), "the two neighbours of every seam row are of different classes"
        first = np.concatenate([[0], np.cumsum(table[1])[:-1]]).tolist()
        for row in laid:
            a, b = first.index(row - 10), first.index(row)
            assert (table[1][a], table[2][a], table[3][a]) == (10, 5, 10) and table[1][b] == 2
            assert table[4][a] * table[1][b] != table[4][b] * table[1][a], "and of different shares of the set"
    recs = _shape("span", 100_003, 8)
    table = mnp.barcode_metrics(recs)
    long = int(np.argmax(table[1]))
    a = int(table[1][:long].sum())
    assert a < 1 + SEG and a + int(table[1][long]) > 1 + 4 * SEG and table[2][long] > 20 and table[3][long] > 3000, "three whole segments"
    recs = _shape("random", 100_003, 0)
    table = mnp.barcode_metrics(recs)
    assert 90 <= int((table[1] > 100).sum()) <= 400 and len(table[0]) > 3000
    data = set(np.unique(recs.view(np.uint64).reshape(-1, 3)[:, 1:]).tolist())
    for values, bits in SETS[1:]:
        assert bits in data and bits - 1 in values, "the value set_bits is in the data, the top bit is set"
    assert (1 << 32) + 7 in data and all(7 in (values or []) for values, bits in SETS[2:]), "2^32 + 7 must not pass for 7"


def _neighbours(n):
    """Four neighbouring barcodes around every seam row, of the classes PASS, LOW | HIGH, SET under _NEIGHBOUR_LIMITS: the first two
    in front of the row, the last two on and behind it."""
    r, w = _base(n)
    rows = []
    for k, s in enumerate(sorted({s for s, _ in SEAM_ROWS})):
        if s - 12 < 0 or s + 14 > n:
            continue
        big = (1 << 42) + 4 * k
        w[s - 12:s + 14, 2] = 5
        w[s - 12:s - 6, 0], w[s - 12:s - 6, 1] = big, [0, 1, 62, 63, 65, 65]            # 6 reads, 5 pairs, 2 of 6 reads in the set: PASS (equality)
        w[s - 6:s, 0], w[s - 6:s, 1] = big + 1, [0, 0, 0, 65, 65, 65]                    # 2 pairs: LOW
        w[s:s + 8, 0], w[s:s + 8, 1] = big + 2, [1, 7, 62, 63, 64, 65, 66, 67]          # 8 pairs: HIGH
        w[s + 8:s + 14, 0], w[s + 8:s + 14, 1] = big + 3, [1, 7, 7, 64, 65, 67]         # 5 pairs, 3 of 6 reads in the set: SET
        rows.append(s)
    return r, rows


_NEIGHBOUR_LIMITS = mnp.limits(min_pairs=3, max_pairs=7, set_num=1, set_den=3)


@pytest.mark.parametrize("skew", SKEWS)
def test_four_classes_on_neighbouring_barcodes(ia, ctx, skew):
    n = 12 * SEG + 300
    recs, rows = _neighbours(n)
    rows = [s + skew // 8 for s in rows]                          # the seams of the walk lie behind the one record a skewed base peels
    recs = np.concatenate([recs[-(skew // 8):], recs[:n - skew // 8]]) if skew else recs
    words = mnp.bitmap([1, 7, 62], 64)
    cls, tot = mnp.filter_barcodes(recs, words, 64, 1, _NEIGHBOUR_LIMITS)
    assert len(rows) == 6
    for s in rows:
        assert cls[s - 12:s + 14].tolist() == [mnp.PASS] * 6 + [mnp.LOW] * 6 + [mnp.HIGH] * 8 + [mnp.SET] * 6, s
    ar = _arena(ia, ctx, 24 * n, n, 8)
    try:
        d, d_class, d_set = ar.carve(24 * n, skew), ar.carve(n, 1), ar.carve(8, 0)
        d.upload(recs)
        d_set.upload(words)
        assert _filter(ia, ctx, d, n, d_set, 64, 1, _NEIGHBOUR_LIMITS, d_class) == tot
        assert d_class.download(np.uint8, n).tobytes() == cls.tobytes()
        ar.check("neighbours")
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        ar.free()


def test_unsorted_input_is_the_run_level_answer(ia, ctx):
    n = 100_003
    recs = _shape("random", n, 0)[np.random.default_rng(0x41500).permutation(n)]
    assert len(mnp.barcode_metrics(recs)[0]) > 5 * len(mnp.barcode_metrics(_shape("random", n, 0))[0])
    _check_case(ia, ctx, recs, n, 8, full=False)


def test_forms_of_the_calls(ia, ctx):
    n = 100_003
    recs = _shape("random", n, 0)
    values, bits = SETS[3]
    words = mnp.bitmap(values, bits)
    table = mnp.barcode_metrics(recs, words, bits, 1)
    B = len(table[0])
    lim = _limit_sets(table, 1)[2]
    cls, tot = mnp.filter_barcodes(recs, words, bits, 1, lim, table)
    ar = _arena(ia, ctx, 24 * n, n, 16, *[8 * B] * 6)
    other = ia.Context(0)
    try:
        d, d_class, d_set = ar.carve(24 * n, 8), ar.carve(n, 1), ar.carve(16, 8)
        cols = [ar.carve(8 * B, 0) for _ in range(6)]
        d.upload(recs)
        d_set.upload(words)
        pattern = np.full(n, PATTERN, np.uint8).tobytes()
        wrap = lambda buf, off: ia.DeviceBuffer.wrap(ctx, buf.ptr + off, 8)
        # every invalid argument is refused before anything is touched, *n_barcodes and the totals included
        bad_sets = [(d_set, bits, 0), (d_set, bits, 3), (d_set, (1 << 32) + 1, 1), (None, 1, 1), (wrap(d_set, 4), 64, 1)]
        for k, (s, b, word) in enumerate(bad_sets):
            nb = C.c_size_t(GARBAGE)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_barcode_metrics(ctx._c, _p(d), n, _p(s), b, word, *[_p(c) for c in cols], B, C.byref(nb), None))
            assert ei.value.kind == "InvalidArg" and nb.value == GARBAGE, k
        for k, (buf, count, col0) in enumerate([(None, 1, cols[0]), (wrap(d, 4), 1, cols[0]), (d, 1 << 40, cols[0]), (d, n, wrap(cols[0], 4))]):
            nb = C.c_size_t(GARBAGE)
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_barcode_metrics(ctx._c, _p(buf), count, _p(d_set), bits, 1, _p(col0), *[_p(c) for c in cols[1:]], B, C.byref(nb), None))
            assert ei.value.kind == "InvalidArg" and nb.value == GARBAGE, k
        with pytest.raises(ia.IbuError):
            ia._check(ia.lib.ibu_barcode_metrics(ctx._c, _p(d), n, _p(d_set), bits, 1, *[_p(c) for c in cols], B, None, None))
        from ibu_amd import _lib
        bad_lims = [mnp.limits(set_of=2), mnp.limits(set_num=2, set_den=1), mnp.limits(set_num=1, set_den=1 << 24), None]
        calls = [(d, n, s, b, word, lim) for s, b, word in bad_sets] + [(d, n, d_set, bits, 1, l) for l in bad_lims] + \
                [(d, 0, d_set, bits, 1, bad_lims[0]), (d, 0, d_set, bits, 3, lim), (None, 1, d_set, bits, 1, lim), (wrap(d, 4), 1, d_set, bits, 1, lim),
                 (d, 1 << 40, d_set, bits, 1, lim)]
        for k, (buf, count, s, b, word, l) in enumerate(calls):
            c = _garbage_counts()
            cl = _lib.CBarcodeLimits(*[l[f] for f in mnp.LIMITS]) if l else None
            with pytest.raises(ia.IbuError) as ei:
                ia._check(ia.lib.ibu_filter_barcodes(ctx._c, _p(buf), count, _p(s), b, word, C.byref(cl) if cl else None, _p(d_class), C.byref(c), None))
            assert ei.value.kind == "InvalidArg", k
            assert [c.barcodes, *c.barcodes_by_class, *c.reads_by_class, c.triples_passed, c.set_triples_passed, c.reserved] == [GARBAGE] * 12, k
        ar.check("refused calls")
        assert d_class.download(np.uint8, n).tobytes() == pattern, "a refused call writes nothing"
        assert all(c.download(np.uint8, 8 * B).tobytes() == np.full(8 * B, PATTERN, np.uint8).tobytes() for c in cols)
        # n == 0: nothing touched, everything 0
        assert _metrics(ia, ctx, None, 0, None, 0, 1, cols, B) == 0
        assert _filter(ia, ctx, None, 0, d_set, bits, 2, lim, d_class) == dict(dict.fromkeys(mnp.TOTALS, 0), barcodes_by_class=(0,) * 4, reads_by_class=(0,) * 4)
        # totals only; neither; classes only, twice on one context (the scratch is reused), then on a stream of another context
        assert _filter(ia, ctx, d, n, d_set, bits, 1, lim, None) == tot
        assert _filter(ia, ctx, d, n, d_set, bits, 1, lim, None, want_counts=False) is None
        ctx.synchronize()
        ar.check("totals only, neither")
        assert d_class.download(np.uint8, n).tobytes() == pattern
        for _ in range(2):
            assert _filter(ia, ctx, d, n, d_set, bits, 1, lim, d_class, want_counts=False) is None
            ar.check("classes only")
            assert d_class.download(np.uint8, n).tobytes() == cls.tobytes()
        want = mnp.filter_barcodes(recs, words, bits, 2, _NEIGHBOUR_LIMITS)
        assert _filter(ia, ctx, d, n, d_set, bits, 2, _NEIGHBOUR_LIMITS, d_class, stream=other.stream) == want[1]
        other.synchronize(other.stream)
        assert d_class.download(np.uint8, n).tobytes() == want[0].tobytes()
        assert _metrics(ia, ctx, d, n, d_set, bits, 1, cols, B, stream=other.stream) == B
        other.synchronize(other.stream)
        ar.check("another stream")
        assert all(c.download(np.uint64, B).tobytes() == t.tobytes() for c, t in zip(cols, table))
        # the Python wrapper
        fs = ctx.feature_bitmap(values, bits)
        assert fs[1] == bits and fs[0].download(np.uint64, 2).tobytes() == words.tobytes()
        got = ctx.barcode_metrics(d, n, fs, 1)
        assert isinstance(got, ia.BarcodeMetrics) and all(g.tobytes() == t.tobytes() for g, t in zip(got, table))
        assert all(g.tobytes() == t.tobytes() for g, t in zip(ctx.barcode_metrics(d, n, None, 2), mnp.barcode_metrics(recs, None, 0, 2)))
        assert all(len(c) == 0 for c in ctx.barcode_metrics(None, 0))
        kw = {k: v for k, v in lim.items() if k.startswith(("min_", "max_"))}
        buf, counts = ctx.filter_barcodes(d, n, fs, 1, max_set_fraction=(lim["set_num"], lim["set_den"]), set_of=("reads", "triples")[lim["set_of"]], **kw)
        ctx.synchronize()
        assert counts == ia.BarcodeFilterCounts(**{k: v for k, v in tot.items() if k != "reserved"}) and buf.download(np.uint8, n).tobytes() == cls.tobytes()
        buf.free()
        assert ctx.filter_barcodes(d, n, fs, 1, d_class=False)[1].barcodes_by_class == (B, 0, 0, 0)
        assert ctx.filter_barcodes(d, n, fs, 1, min_pairs=2, d_class=False, counts=False) == (None, None)
        fs[0].free()
        assert d.download(count=24 * n).tobytes() == recs.tobytes()
    finally:
        other.close()
        ar.free()


@pytest.mark.parametrize("n", [2561, 100_003])
def test_cross_checks_against_the_other_aggregations(ia, ctx, n):
    """On the same array: reads and pairs are ibu_barcode_counts' counts and unique_umis, the triples add up to ibu_pair_counts'
    n_triples, and ibu_select_records on the class bytes is the numpy subset — on records that went through the swap and the sort,
    what the count matrix leaves."""
    rng = np.random.default_rng(0x41600 + n)
    recs = _shape("random", n, 0)[rng.permutation(n)]
    swapped = recs.copy()
    swapped["umi"], swapped["index"] = recs["index"], recs["umi"]
    want = count_np.sort_records(swapped)
    d, tmp = ctx.upload(recs), ctx.alloc(24 * n)
    ctx.swap_umi_index(d, d, n)
    ctx.sort_records(d, tmp, n)
    ctx.synchronize()
    assert d.download(mnp.REC, n).tobytes() == want.tobytes()
    values, bits = SETS[2]
    fs = ctx.feature_bitmap(values, bits)
    got = ctx.barcode_metrics(d, n, fs, 1)
    table = mnp.barcode_metrics(want, mnp.bitmap(values, bits), bits, 1)
    assert all(g.tobytes() == t.tobytes() for g, t in zip(got, table))
    b, c, u = ctx.barcode_counts(d, n)
    assert b.tobytes() == got.barcodes.tobytes() and c.tobytes() == got.reads.tobytes() and u.tobytes() == got.pairs.tobytes()
    npairs, ntriples = C.c_size_t(), C.c_size_t()
    ia._check(ia.lib.ibu_pair_counts(ctx._c, _p(d), n, None, None, None, None, 0, C.byref(npairs), C.byref(ntriples), None))
    assert int(got.triples.sum()) == ntriples.value and int(got.pairs.sum()) == npairs.value
    lim = _limit_sets(table, 1)[2]
    cls, tot = mnp.filter_barcodes(want, mnp.bitmap(values, bits), bits, 1, lim, table)
    assert 0 < tot["reads_by_class"][0] < n
    d_class, counts = ctx.filter_barcodes(d, n, fs, 1, max_set_fraction=(lim["set_num"], lim["set_den"]), set_of=("reads", "triples")[lim["set_of"]],
                                          **{k: v for k, v in lim.items() if k.startswith(("min_", "max_"))})
    assert counts.reads_by_class == tot["reads_by_class"]
    out, k = ctx.select_records(d, d_class, n, 1 << ia.BARCODE_PASS)
    ctx.synchronize()
    assert k == tot["reads_by_class"][0] and out.download(mnp.REC, k).tobytes() == want[cls == mnp.PASS].tobytes(), "the passing barcodes, still sorted"
    assert int(ctx.barcode_metrics(out, k, fs, 1).triples.sum()) == tot["triples_passed"]
    for x in (d, tmp, d_class, out, fs[0]):
        x.free()


def test_count_file_qc(ia, tmp_path):
    """examples/count_file.cpp --qc --set end to end: the matrix of the barcodes that pass, counted without a second sort."""
    import os
    import subprocess
    from ibu_amd import _lib
    from tests import cells_np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "count_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "count_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len = 16
    rng = np.random.default_rng(0x41700)
    recs = cells_np.knee(rng, 30, 200, cell_umis=(50, 100), reads_per_umi=2)
    recs["index"] = (recs["umi"] * np.uint64(7) + recs["barcode"]) % (np.uint64(20) + recs["barcode"] % np.uint64(25))   # 20 .. 44 features
    recs = recs[rng.permutation(len(recs))]
    n = len(recs)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    in_set = [3, 5, 39]
    (tmp_path / "set.txt").write_text("".join(f"{v}\n" for v in in_set))
    swapped = recs.copy()
    swapped["umi"], swapped["index"] = recs["index"], recs["umi"]
    swapped = count_np.sort_records(swapped)
    lim = mnp.limits(min_pairs=10, max_pairs=35, min_triples=20, set_num=1, set_den=12, set_of=1)
    cls, tot = mnp.filter_barcodes(swapped, mnp.bitmap(in_set, 40), 40, 1, lim)
    assert all(tot["barcodes_by_class"]), tot
    kept = swapped[cls == mnp.PASS]
    kept["umi"], kept["index"] = kept["index"].copy(), kept["umi"].copy()
    b, i, reads, umis = count_np.brute_force_matrix(kept)
    text = lambda c: "".join("ACGT"[(int(c) >> (2 * k)) & 3] for k in range(bc_len))
    r = subprocess.run([str(exe), "--qc=minfeat:10,maxfeat:35,minumi:20,maxset:1/12", f"--set={tmp_path / 'set.txt'}", str(tmp_path / "in.ibu")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    matrix = [l for l in r.stdout.splitlines() if not l.startswith("#")]
    assert matrix == [f"{text(bb)}\t{ii}\t{uu}\t{rr}" for bb, ii, rr, uu in zip(b.tolist(), i.tolist(), reads.tolist(), umis.tolist())]
    bc, rc = tot["barcodes_by_class"], tot["reads_by_class"]
    assert (f"{n} records: barcodes {tot['barcodes']}: pass {bc[0]}, low {bc[1]}, high {bc[2]}, set {bc[3]}; "
            f"reads pass {rc[0]}, low {rc[1]}, high {rc[2]}, set {rc[3]}") in r.stderr
    rows = [l.split("\t") for l in r.stdout.splitlines() if l.startswith("#row")]
    assert len(rows) == bc[0] and sum(int(x[3]) for x in rows) == rc[0]


def test_more_than_1024_segments(ia, ctx):
    """9.5e6 records are 1160 segments: the scan of the per-segment counters takes a second round of 1024, and the barcodes that
    begin behind segment 1024 (two of the fourteen), their prefix rows and their records' class bytes rest on what it carries over."""
    n, length = 9_500_000, 700_001
    assert n // SEG > 1024 and 12 * length > 1024 * SEG + 1
    i = np.arange(n, dtype=np.int64)
    recs = np.zeros(n, mnp.REC)
    w = recs.view(np.uint64).reshape(-1, 3)
    w[:, 0], w[:, 1], w[:, 2] = (i // length + 3).astype(np.uint64), PALETTE[(i // 5 + i // length) % 8], PALETTE[(i // 2) % 8]
    values, bits = SETS[3]
    words = mnp.bitmap(values, bits)
    table = mnp.barcode_metrics(recs, words, bits, 1)
    B = len(table[0])
    lim = mnp.limits(max_reads=length - 1, set_num=int(table[5][-1]), set_den=int(table[3][-1]), set_of=1)   # the last barcode is shorter, and sits on the bound: PASS
    assert B == 14 and lim["set_den"] < 1 << 24
    cls, tot = mnp.filter_barcodes(recs, words, bits, 1, lim, table)
    assert tot["barcodes_by_class"][0] >= 1 and tot["barcodes_by_class"][2] >= 12
    for skew in SKEWS:
        buf = ctx.alloc(24 * n + 16)
        d = ia.DeviceBuffer.wrap(ctx, buf.ptr + skew, 24 * n)
        d.upload(recs)
        fs = ctx.feature_bitmap(values, bits)
        got = ctx.barcode_metrics(d, n, fs, 1)
        assert all(g.tobytes() == t.tobytes() for g, t in zip(got, table)), skew
        d_class = ctx.alloc(n)
        assert _filter(ia, ctx, d, n, fs[0], bits, 1, lim, d_class) == tot
        ctx.synchronize()
        assert d_class.download(np.uint8, n).tobytes() == cls.tobytes(), skew
        for x in (buf, d_class, fs[0]):
            x.free()
