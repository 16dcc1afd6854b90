"""The statement the census seam tests compare the device with (tests/census_np.py), pinned without a GPU: its flags against the
oracle's order, its base, its defects, its seam rows and its shortcut for patched arrays against the plain pass over all rows."""
import numpy as np
import pytest

from tests import census_np as cn
from tests import keyplan_np as kp


def _random(rng, n, spread):
    recs = np.zeros(n, dtype=cn.REC)
    for f in kp.FIELDS:
        recs[f] = rng.integers(0, spread, n, dtype=np.uint64)
    return recs


def _flags_by_hand(recs):
    """The same two questions with Python integers and tuples."""
    rows = [(int(r["barcode"]), int(r["umi"]), int(r["index"])) for r in recs]
    return (any(b[2] < a[2] for a, b in zip(rows, rows[1:])), any(b < a for a, b in zip(rows, rows[1:])))


@pytest.mark.parametrize("spread", [2, 5, 300, 2**64])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 50, 1000])
def test_flags_against_the_oracle_on_random_records(oracle, n, spread):
    rng = np.random.default_rng(n + 7)
    for recs in (_random(rng, n, spread), oracle.sort_records(_random(rng, n, spread))):
        idx, order = cn.flags(recs)
        assert (idx, order) == _flags_by_hand(recs)
        assert order == (not oracle.is_sorted(recs)) == (oracle.sort_records(recs).tobytes() != recs.tobytes())
        in_index_order = recs.copy()
        in_index_order["index"] = np.sort(recs["index"])
        assert cn.flags(in_index_order)[0] is False
        assert cn.words(recs) == kp.census_words(recs)


def test_values_from_2_pow_63_on_compare_as_unsigned(oracle):
    top = 1 << 63
    for f, want in (("barcode", (False, True)), ("umi", (False, True)), ("index", (True, True))):
        recs = np.zeros(2, dtype=cn.REC)
        recs[f] = [top, top - 1]                              # falls; as signed 64-bit it would rise
        assert cn.flags(recs) == want == _flags_by_hand(recs), f
        assert oracle.is_sorted(recs) is False
        recs[f] = [top - 1, top]                              # rises; as signed it would fall
        assert cn.flags(recs) == (False, False), f
        assert oracle.is_sorted(recs) is True
        recs[f] = [2**64 - 1, top + 5]
        assert cn.flags(recs) == want, f
    recs = np.zeros(2, dtype=cn.REC)
    recs["index"] = [(1 << 53) + 1, 1 << 53]                  # a difference that float64 does not see
    assert cn.flags(recs) == (True, True)


@pytest.mark.parametrize("n", list(cn.SMALL_SIZES) + [5000])
def test_clean_base_is_sorted_in_index_order_and_has_room(oracle, n):
    base = cn.clean_base(n, n)
    assert cn.flags(base) == (False, False) and oracle.is_sorted(base)
    assert base.tobytes() == oracle.sort_records(base).tobytes()
    w_or, w_and = cn.words(base)
    for k, f in enumerate(kp.FIELDS):
        assert w_or[k] < 1 << 62
        assert w_and[k] & cn.FIXED[f] == cn.FIXED[f]          # the fixed bits: in every record
        assert not w_or[k] >> cn.OUTLIER_SET[f] & 1 and w_and[k] >> cn.OUTLIER_CLEAR[f] & 1
    assert (np.diff(base["index"].astype(np.int64)) == 4).all()
    if n >= 5000:
        runs = np.diff(np.flatnonzero(np.diff(base["barcode"].astype(np.int64)) != 0))
        assert runs.min() == 1 and runs.max() == cn.RUN_MAX   # ties on the barcode, and no run longer than a patch can renumber
        same = base["barcode"][1:] == base["barcode"][:-1]
        assert (base["umi"][1:] == base["umi"][:-1])[same].any() and (base["umi"][1:] > base["umi"][:-1])[same].any()


@pytest.mark.parametrize("kind", cn.KINDS)
def test_every_defect_kind_is_one_defect_on_one_pair(oracle, kind):
    """At every row of a base, and at every seam row of every size: the patch touches at most three neighbouring records, the pair
    (p - 1, p) is the only one with a drop and has exactly the drops of its kind, and Base.expect — the statement on the patched
    neighbourhood — equals the statement and the oracle on the whole patched array."""
    cases = [(200, 0, p) for p in range(1, 200)]
    cases += [(n, peeled, p) for n in cn.SMALL_SIZES for peeled in (0, 1) for p, _ in cn.seams(n, peeled)]
    bases = {}
    for n, peeled, p in cases:
        base = bases.setdefault(n, cn.Base(cn.clean_base(n, n)))
        patch = cn.plant(base.recs, p, kind)
        full = cn.apply(base.recs, patch)
        idx_rows, order_rows = cn.drop_rows(full)
        want_idx, want_order = cn.KIND_FLAGS[kind]
        assert idx_rows.tolist() == ([p] if want_idx else []), (n, p)
        assert order_rows.tolist() == ([p] if want_order else []), (n, p)
        assert oracle.is_sorted(full) == (not want_order)
        e = base.expect(patch)
        assert (e["index_drops"], e["order_drops"]) == cn.flags(full) == (want_idx, want_order)
        assert (e["or"], e["and"]) == cn.words(full)
        a, b = full[p - 1], full[p]
        if kind.endswith("h"):                                # the fall is in the high halves only, the low halves rise
            f = {"1h": "index", "3h": "barcode", "4h": "umi"}[kind]
            assert int(b[f]) >> 32 < int(a[f]) >> 32 and int(b[f]) & 0xFFFFFFFF > int(a[f]) & 0xFFFFFFFF
        if kind.endswith("s"):
            f = {"1s": "index", "3s": "barcode", "4s": "umi"}[kind]
            assert int(b[f]) < 1 << 63 <= int(a[f])
        if kind == "6":
            assert a.tobytes() == b.tobytes()
        if kind in ("2", "5"):
            assert int(b["barcode"]) > int(a["barcode"]) and (int(b["index"]) < int(a["index"]) if kind == "2" else int(b["umi"]) < int(a["umi"]))


@pytest.mark.parametrize("n", [133, 3 * 128 + 37, 1 + 3 * 128 + 37])
def test_outlier_bits_change_exactly_one_word_bit(n):
    base = cn.Base(cn.clean_base(n, n))
    w_or, w_and = cn.words(base.recs)
    for peeled in (0, 1):
        for row, _ in cn.outlier_rows(n, peeled):
            for k, f in enumerate(kp.FIELDS):
                for clear in (False, True):
                    patch = cn.plant_bit(base.recs, row, f, clear)
                    e = base.expect(patch)
                    full = cn.apply(base.recs, patch)
                    assert (e["or"], e["and"]) == cn.words(full) and (e["index_drops"], e["order_drops"]) == cn.flags(full)
                    want_or, want_and = list(w_or), list(w_and)
                    if clear:
                        want_and[k] &= ~(1 << cn.OUTLIER_CLEAR[f])
                    else:
                        want_or[k] |= 1 << cn.OUTLIER_SET[f]
                    assert (e["or"], e["and"]) == (want_or, want_and)
                    assert kp.Plan(e["or"], e["and"]).k == kp.Plan(w_or, w_and).k + 1   # the byte of that bit varies now, and only there


def test_seam_rows_follow_the_split():
    assert cn.split(0, 1) == (0, 0, 0) and cn.split(1, 1) == (1, 0, 0) and cn.split(129, 1) == (1, 128, 0) and cn.split(129, 0) == (0, 128, 1)
    assert dict(cn.seams(2, 0)) == {1: "row 1 = last row"} and dict(cn.seams(2, 1)) == {1: "row 1 = peel/tile = main/rest = last row"}
    n = 1 + 3 * 128 + 37
    assert [p for p, _ in cn.seams(n, 0)] == [1, 2, 63, 64, 65, 126, 127, 128, 256, 384, n - 1]
    assert [p for p, _ in cn.seams(n, 1)] == [1, 2, 3, 64, 65, 66, 127, 128, 129, 257, 385, n - 1]
    assert dict(cn.seams(n, 1))[385] == "tile seam 3 = main/rest" and dict(cn.seams(n, 1))[257] == "tile seam 2 = last tile"
    assert cn.left_out(n, 1) == ["rest wave edge"] and cn.left_out(n, 0) == ["peel/tile", "rest wave edge"]
    assert "rest wave edge" in dict(cn.seams(128 + 70, 0))[128 + 64]
    for n in list(cn.SMALL_SIZES) + [cn.LARGE_SIZE]:
        for peeled in (0, 1):
            head, main, rest = cn.split(n, peeled)
            assert head + main + rest == n and main % cn.TILE == 0 and rest < cn.TILE and head == peeled
            assert len(cn.seam_candidates(n, peeled)) == 9 + len(cn.IN_TILE)
            rows = [p for p, _ in cn.outlier_rows(n, peeled)]
            assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == n - 1 and head + main in rows + [n]
    # what the sizes of the GPU file cannot express: no tile at all, a rest too short for a second wave, row 0 of an unpeeled array
    assert sum(len(cn.left_out(n, peeled)) for n in cn.SMALL_SIZES + (cn.LARGE_SIZE,) for peeled in (0, 1)) == 187
    assert cn.tile_seams(1000, 1, [0, 3, 3, 6]) == [(1, "tile 0"), (385, "tile 3"), (769, "tile 6")]
    assert cn.tile_seams(1000, 0, [0, 6]) == [(768, "tile 6")]
