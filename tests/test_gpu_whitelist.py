"""Barcode correction against a whitelist on the device (ibu_whitelist_create, ibu_correct_barcodes, ibu_select_records):
every comparison is byte for byte against the numpy statement of the semantics in tests/whitelist_np.py."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import whitelist_np as wnp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 63, 127, 128, 129, 255, 2559, 2561, 5121, 100_003]   # tests/test_gpu_guards.py
NS = SIZES + [1_000_003]
BC_LENS = [1, 4, 10, 16, 31, 32]
WS = [1, 2, 1000, 100_000]
GRID = list(itertools.product(BC_LENS, WS, NS))
CASES = [(b, w, n) for b, w, n in GRID if 4 ** b >= w]              # the only pruning: a whitelist larger than the code space
assert len(GRID) - len(CASES) < len(GRID) / 5, (len(GRID), len(CASES))
GUARD, PATTERN = 4096, 0xA5


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


class Arena:
    """One allocation, pattern-filled; carve(nbytes, skew) hands out a view that starts `skew` bytes behind a 256-byte
    boundary with at least GUARD pattern bytes on either side; check() looks at every byte outside the views
    (the helper of tests/test_gpu_guards.py)."""

    def __init__(self, ia, ctx, total):
        self.ia, self.ctx = ia, ctx
        self.total = total
        self.buf = ctx.upload(np.full(total, PATTERN, np.uint8))
        self.pos = GUARD
        self.used = []

    def carve(self, nbytes, skew=0):
        start = (self.pos + 255) // 256 * 256 + skew
        assert start + nbytes + GUARD <= self.total, "arena too small"
        self.used.append((start, start + nbytes))
        self.pos = start + nbytes + GUARD
        return self.ia.DeviceBuffer.wrap(self.ctx, self.buf.ptr + start, max(nbytes, 1))

    def check(self, what):
        self.ctx.synchronize()
        host = self.buf.download(np.uint8)
        mask = np.ones(self.total, bool)
        for a, b in self.used:
            mask[a:b] = False
        bad = np.flatnonzero(mask & (host != PATTERN))
        assert bad.size == 0, f"{what}: {bad.size} guard bytes overwritten, first at arena offset {int(bad[0])} (views: {self.used})"

    def free(self):
        self.buf.free()


def _arena(ia, ctx, *sizes):
    return Arena(ia, ctx, sum(sizes) + (len(sizes) + 2) * (GUARD + 512) + 4096)


def _records(rng, bc):
    recs = np.zeros(len(bc), wnp.REC)
    recs["barcode"] = bc
    recs["umi"] = rng.integers(0, 1 << 63, len(bc), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(bc), dtype=np.uint64)
    recs["index"] = np.arange(len(bc), dtype=np.uint64)
    return recs


@functools.lru_cache(maxsize=4)
def _case(bc_len, w):
    """The largest input of a (bc_len, w) cell and its numpy answer; the smaller sizes are prefixes (the mix is shuffled)."""
    rng = np.random.default_rng(0x1B00300 + 1000 * bc_len + w % 997)
    wl, bc = wnp.make_case(rng, bc_len, w, max(NS))
    recs = _records(rng, bc)
    want, cls, _ = wnp.correct_records(recs, wl, bc_len, 1)
    return wl, recs, want, cls


def _whitelist(ia, ctx, wl, bc_len):
    d = ctx.upload(np.ascontiguousarray(wl, dtype=np.uint64))
    try:
        return ia.Whitelist(ctx, d, len(wl), bc_len)
    finally:
        d.free()


def _counts(cls):
    n = np.bincount(cls, minlength=4)
    return {"exact": int(n[0]), "corrected": int(n[1]), "ambiguous": int(n[2]), "unmatched": int(n[3])}


def _check_untouched(got, recs, cls, bc_len):
    m = wnp.mask(bc_len)
    assert (got["umi"] == recs["umi"]).all() and (got["index"] == recs["index"]).all()
    assert ((got["barcode"] & ~m) == (recs["barcode"] & ~m)).all()
    assert got[cls != 1].tobytes() == recs[cls != 1].tobytes()


@pytest.mark.parametrize("bc_len,w,n", CASES)
def test_correct_matches_numpy(ia, ctx, bc_len, w, n):
    wl, recs, want, cls = _case(bc_len, w)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    with _whitelist(ia, ctx, wl, bc_len) as h:
        assert h.bc_len == bc_len and h.n_distinct == len(np.unique(wl)) and h.device_bytes >= 16 * h.n_distinct
        d, d_cls = ctx.upload(recs), ctx.alloc(max(n, 16))
        got_counts = ctx.correct_barcodes(h, d, n, 1, d_cls)
        got, got_cls = d.download(wnp.REC, n), d_cls.download(np.uint8, n)
        d.free(); d_cls.free()
    assert got_counts == _counts(cls)
    assert (got_cls == cls).all()
    assert got.tobytes() == want.tobytes()
    _check_untouched(got, recs, cls, bc_len)


def test_large_table_beyond_l2(ia, ctx):
    """3e6 codes (a 64 MiB table, beyond the 32 MiB of aggregate L2), 2e7 records: 94 % exact, 5 % one substitution (some of
    them ambiguous in so dense a whitelist), 1 % uniform random so that class 3 occurs."""
    bc_len, w, n = 16, 3_000_000, 20_000_000
    rng = np.random.default_rng(0x1B00301)
    wl, bc = wnp.make_case(rng, bc_len, w, n, shares=(0.94, 0.05, 0.0, 0.01))
    recs = _records(rng, bc)
    want, cls, counts = wnp.correct_records(recs, wl, bc_len, 1)
    print("class counts", counts)
    assert min(counts.values()) > 0
    with _whitelist(ia, ctx, wl, bc_len) as h:
        assert h.device_bytes >= 64 << 20
        d, d_cls = ctx.upload(recs), ctx.alloc(n)
        got_counts = ctx.correct_barcodes(h, d, n, 1, d_cls)
        got, got_cls = d.download(wnp.REC, n), d_cls.download(np.uint8, n)
        d.free(); d_cls.free()
    assert got_counts == counts
    assert (got_cls == cls).all() and got.tobytes() == want.tobytes()
    _check_untouched(got, recs, cls, bc_len)


def test_forms_of_the_call(ia, ctx):
    """max_mismatches 0; no class bytes; no counts (asynchronous) and a later synchronise; n == 0."""
    bc_len, n = 16, 100_003
    wl, recs, want, cls = _case(bc_len, 1000)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    want0, cls0, counts0 = wnp.correct_records(recs, wl, bc_len, 0)
    assert set(np.unique(cls0)) == {0, 3} and want0.tobytes() == recs.tobytes()
    with _whitelist(ia, ctx, wl, bc_len) as h:
        d, d_cls = ctx.upload(recs), ctx.alloc(n)
        assert ctx.correct_barcodes(h, d, n, 0, d_cls) == counts0
        assert (d_cls.download(np.uint8, n) == cls0).all() and d.download(wnp.REC, n).tobytes() == recs.tobytes()
        assert ctx.correct_barcodes(h, d, n, 1, None) == _counts(cls)                  # d_class = NULL
        assert d.download(wnp.REC, n).tobytes() == want.tobytes()
        d.upload(recs)
        assert ctx.correct_barcodes(h, d, n, 1, d_cls, counts=False) is None           # counts = NULL
        ctx.synchronize()
        assert d.download(wnp.REC, n).tobytes() == want.tobytes() and (d_cls.download(np.uint8, n) == cls).all()
        assert ctx.correct_barcodes(h, d, 0, 1, None) == {"exact": 0, "corrected": 0, "ambiguous": 0, "unmatched": 0}   # n == 0
        d.free(); d_cls.free()


def test_whitelist_order_duplicates_and_base_order(ia, ctx):
    bc_len, n = 10, 100_003
    wl, recs, want, cls = _case(bc_len, 1000)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    rng = np.random.default_rng(5)
    forms = [wl, wl[::-1].copy(), rng.permutation(np.concatenate([wl, wl[:300], wl[:3]]))]
    d, d_cls = ctx.alloc(24 * n), ctx.alloc(n)
    for order in (0, 1):
        ctx.set_option("base_order", order)
        try:
            for f in forms:
                with _whitelist(ia, ctx, f, bc_len) as h:
                    assert h.n_distinct == len(wl)
                    d.upload(recs)
                    assert ctx.correct_barcodes(h, d, n, 1, d_cls) == _counts(cls)
                    assert d.download(wnp.REC, n).tobytes() == want.tobytes() and (d_cls.download(np.uint8, n) == cls).all()
        finally:
            ctx.set_option("base_order", 0)
    d.free(); d_cls.free()


def test_32_bases_with_zero_and_all_ones(ia, ctx):
    """At 32 bases every 64-bit value is a legal code: 0 and ~0 are in the whitelist and among the records."""
    ones = (1 << 64) - 1
    wl = np.array([0, ones, 0x0123456789ABCDEF, ones], np.uint64)
    bc = np.array([0, ones, 1, ones ^ (2 << 62), ones ^ 1, 3 << 62, 0x0123456789ABCDEF ^ (1 << 20), 5, ones ^ 0b0101, 0x0123456789ABCDEF] * 40,
                  np.uint64)
    recs = _records(np.random.default_rng(6), bc)
    want, cls, counts = wnp.correct_records(recs, wl, 32, 1)
    assert (cls == wnp.brute_force(bc, wl, 32)[0]).all() and set(np.unique(cls)) == {0, 1, 3}
    with _whitelist(ia, ctx, wl, 32) as h:
        assert h.n_distinct == 3
        d, d_cls = ctx.upload(recs), ctx.alloc(len(bc))
        assert ctx.correct_barcodes(h, d, len(bc), 1, d_cls) == counts
        assert d.download(wnp.REC, len(bc)).tobytes() == want.tobytes() and (d_cls.download(np.uint8, len(bc)) == cls).all()
        d.free(); d_cls.free()
    with _whitelist(ia, ctx, np.array([7, 9], np.uint64), 32) as h:   # and a 32-base whitelist WITHOUT all ones does not know it
        d = ctx.upload(recs)
        c = ctx.correct_barcodes(h, d, len(bc), 1, None)
        assert c == wnp.correct_records(recs, [7, 9], 32, 1)[2]
        d.free()


def test_two_streams_share_one_whitelist(ia, ctx):
    bc_len, n = 16, 1_000_003
    wl, recs, want, cls = _case(bc_len, 100_000)
    half = n // 2
    other = ia.Context(0)                               # its stream is a second hardware queue on the same device
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h:
            da, db = ctx.upload(recs[:half]), ctx.upload(recs[half:])
            ca, cb = ctx.alloc(half), ctx.alloc(n - half)
            ctx.correct_barcodes(h, da, half, 1, ca, counts=False)
            ctx.correct_barcodes(h, db, n - half, 1, cb, counts=False, stream=other.stream)
            ctx.synchronize()
            ctx.synchronize(other.stream)
            assert da.download(wnp.REC, half).tobytes() == want[:half].tobytes()
            assert db.download(wnp.REC, n - half).tobytes() == want[half:].tobytes()
            assert (ca.download(np.uint8, half) == cls[:half]).all() and (cb.download(np.uint8, n - half) == cls[half:]).all()
            for b in (da, db, ca, cb):
                b.free()
    finally:
        other.close()


def test_argument_errors(ia, ctx):
    codes = ctx.upload(np.array([1, 2, 1 << 20, 3, 1 << 21], np.uint64))
    with pytest.raises(ia.IbuError) as ei:
        ia.Whitelist(ctx, codes, 5, 10)                 # bit 20 is at 2*bc_len
    assert ei.value.kind == "InvalidArg" and ei.value.a == 2
    for w, bc_len in ((0, 10), (2, 0), (2, 33)):
        with pytest.raises(ia.IbuError) as ei:
            ia.Whitelist(ctx, codes, w, bc_len)
        assert ei.value.kind == "InvalidArg", (w, bc_len)
    other = ia.Context(0)
    try:
        with ia.Whitelist(ctx, codes, 2, 10) as h:
            d = ctx.upload(np.zeros(4, wnp.REC))
            with pytest.raises(ia.IbuError) as ei:
                ctx.correct_barcodes(h, d, 4, 2)
            assert ei.value.kind == "InvalidArg"
            d2 = other.upload(np.zeros(4, wnp.REC))
            with pytest.raises(ia.IbuError) as ei:
                other.correct_barcodes(h, d2, 4, 1)
            assert ei.value.kind == "InvalidArg"
            d.free(); d2.free()
    finally:
        other.close()
    codes.free()


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(7)
    n = 100_003
    cls = rng.choice(np.array([0, 1, 2, 3, 0, 0, 1, 4, 7, 8, 200, 255], np.uint8), n)
    cls[5000:9000] = 2                                   # whole units with nothing / everything kept
    cls[20000:26000] = 0
    return _records(rng, rng.integers(0, 1 << 32, n, dtype=np.uint64)), cls


@pytest.mark.parametrize("keep", range(16))
def test_select_every_mask(ia, ctx, mixed, keep):
    recs, cls = mixed
    n = len(recs)
    d, d_cls = ctx.upload(recs), ctx.upload(cls)
    out, k = ctx.select_records(d, d_cls, n, keep)
    want = recs[np.isin(cls, [c for c in range(4) if (keep >> c) & 1])]
    assert k == len(want)
    if k:
        assert out.download(wnp.REC, k).tobytes() == want.tobytes()
    for b in (d, d_cls, out):
        b.free()


def test_select_forms(ia, ctx, mixed):
    """Size query; classes 4..255 are never kept whatever the mask says above bit 7; n == 0; cap too small."""
    recs, cls = mixed
    n = len(recs)
    lib = ia.lib
    d, d_cls = ctx.upload(recs), ctx.upload(cls)
    k = C.c_size_t(99)
    assert lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, 0b0011, None, 0, C.byref(k), None) == 0
    assert k.value == int(np.isin(cls, [0, 1]).sum())
    out, k_all = ctx.select_records(d, d_cls, n, 0xFFFFFFFF)
    want = recs[cls < 8]
    assert k_all == len(want) and out.download(wnp.REC, k_all).tobytes() == want.tobytes()
    assert lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, 0, 0b0011, None, 0, C.byref(k), None) == 0 and k.value == 0
    ar = _arena(ia, ctx, 24 * 100)
    try:
        small = ar.carve(24 * 100)
        rc = lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, 0b0011, small.ptr, 100, C.byref(k), None)
        assert rc != 0 and lib.ibu_status_name(rc) == b"InvalidArg" and k.value == int(np.isin(cls, [0, 1]).sum())
        ar.check("select with too small a capacity")
        assert (small.download(np.uint8, 2400) == PATTERN).all()          # d_out untouched
    finally:
        ar.free()
    rc = lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, 0b0011, d.ptr + 24 * 10, n, C.byref(k), None)
    assert rc != 0 and lib.ibu_status_name(rc) == b"InvalidArg"             # overlap
    for b in (d, d_cls, out):
        b.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("skew", [0, 8])
def test_buffers_at_their_contract_sizes(ia, ctx, n, skew):
    """d_records (24 n), d_class (n) and d_out (24 x kept) carved out of a guarded arena, 8- but not 16-byte aligned too."""
    bc_len = 16
    wl, recs, want, cls = _case(bc_len, 1000)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    kept = want[np.isin(cls, [0, 1])]
    ar = _arena(ia, ctx, 24 * n, n, 24 * len(kept))
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h:
            d = ar.carve(24 * n, skew)
            d.upload(recs)
            d_cls = ar.carve(n, 1 if skew else 0)                          # class bytes need no alignment
            d_out = ar.carve(24 * len(kept), skew)
            assert ctx.correct_barcodes(h, d, n, 1, d_cls) == _counts(cls)
            k = C.c_size_t()
            ia._check(ia.lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, 0b0011, d_out.ptr if len(kept) else None, len(kept), C.byref(k), None))
            ar.check(f"correct + select n={n} skew={skew}")
            assert k.value == len(kept)
            assert d.download(count=24 * n).tobytes() == want.tobytes() and (d_cls.download(np.uint8, n) == cls).all()
            if len(kept):
                assert d_out.download(count=24 * len(kept)).tobytes() == kept.tobytes()
            d.upload(recs)                                                 # the same array without class bytes: peeled head + NULL
            assert ctx.correct_barcodes(h, d, n, 1, None) == _counts(cls)
            ar.check(f"correct without class bytes n={n} skew={skew}")
            assert d.download(count=24 * n).tobytes() == want.tobytes()
    finally:
        ar.free()


def _noisy_file_case(n, w, bc_len, seed):
    rng = np.random.default_rng(seed)
    wl, bc = wnp.make_case(rng, bc_len, w, n, junk=False, shares=(0.94, 0.05, 0.0, 0.01))
    recs = _records(rng, bc)
    recs["umi"] &= wnp.mask(12)
    return wl, recs


def _numpy_chain(recs, wl, bc_len, keep=(0, 1)):
    want, cls, counts = wnp.correct_records(recs, wl, bc_len, 1)
    kept = want[np.isin(cls, keep)]
    kept = kept[np.lexsort((kept["index"], kept["umi"], kept["barcode"]))]
    b, c = np.unique(kept["barcode"], return_counts=True)
    return kept, b, c.astype(np.uint64), counts


def test_the_chain_the_feature_exists_for(ia, ctx):
    """records with sequencing errors -> correct -> select exact | corrected -> sort -> per-barcode counts: no more barcodes
    than the whitelist has — which does NOT hold for the uncorrected input."""
    n, w, bc_len = 1_000_000, 4000, 16
    wl, recs = _noisy_file_case(n, w, bc_len, 0x1B00302)
    kept, want_b, want_c, counts = _numpy_chain(recs, wl, bc_len)
    d, tmp = ctx.upload(recs), ctx.alloc(24 * n)
    ctx.sort_records(d, tmp, n)
    raw_b, _, _ = ctx.barcode_counts(d, n, unique_umis=False)
    assert len(raw_b) > w                                               # the uncorrected input overshoots the whitelist bound
    d.upload(recs)
    with _whitelist(ia, ctx, wl, bc_len) as h:
        d_cls = ctx.alloc(n)
        assert ctx.correct_barcodes(h, d, n, 1, d_cls) == counts
    out, k = ctx.select_records(d, d_cls, n, 0b0011)
    assert k == len(kept)
    ctx.sort_records(out, tmp, k)
    assert out.download(wnp.REC, k).tobytes() == kept.tobytes()
    got_b, got_c, _ = ctx.barcode_counts(out, k, unique_umis=False)
    assert len(got_b) <= w
    assert (got_b == want_b).all() and (got_c == want_c).all()
    for b in (d, tmp, d_cls, out):
        b.free()


def test_correct_file_example(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "correct_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "correct_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    n, w, bc_len = 50_000, 500, 16
    wl, recs = _noisy_file_case(n, w, bc_len, 0x1B00303)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    text = ["".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(bc_len)) for c in wl]   # base i at bits [2i, 2i+1]
    (tmp_path / "wl.txt").write_text("\n".join(text) + "\n")
    for flag, keep in (((), (0, 1)), (("--keep-ambiguous",), (0, 1, 2))):
        r = subprocess.run([str(exe), str(tmp_path / "in.ibu"), str(tmp_path / "wl.txt"), str(tmp_path / "out.ibu"), *flag],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        kept, want_b, _, counts = _numpy_chain(recs, wl, bc_len, keep)
        h, got = ia.load_to_vec(str(tmp_path / "out.ibu"))
        assert h.sorted() and np.asarray(got).tobytes() == kept.tobytes()
        assert f"exact {counts['exact']}, corrected {counts['corrected']}, ambiguous {counts['ambiguous']}, unmatched {counts['unmatched']}" in r.stdout
        assert f"after {len(want_b)}" in r.stdout and f"before {len(np.unique(recs['barcode']))}" in r.stdout
