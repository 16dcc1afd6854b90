"""Whitelist abundance and the resolution of ambiguous barcodes on the device (ibu_abundance_add, ibu_abundance_counts,
ibu_resolve_barcodes): every comparison is byte for byte against the numpy statement of the semantics in tests/resolve_np.py —
records, class bytes, the four totals and the counters."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import resolve_np as rnp
from tests import whitelist_np as wnp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 127, 128, 129, 5121, 100_003]
BC_LENS = [5, 16, 22, 32]
WS = [2, 1000, 100_000]
CASES = [(b, w, n) for b, w, n in itertools.product(BC_LENS, WS, NS) if 4 ** b >= w]   # the only pruning: a whitelist larger than the code space
CLASS_SKEWS = [0, 1, 2, 15]
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
    """One allocation, pattern-filled; carve(nbytes, skew) hands out a view that starts `skew` bytes behind a 256-byte boundary
    with at least GUARD pattern bytes on either side; check() looks at every byte outside the views (the helper of
    tests/test_gpu_guards.py)."""

    def __init__(self, ia, ctx, total):
        self.ia, self.ctx, self.total = ia, ctx, total
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


def _whitelist(ia, ctx, wl, bc_len):
    d = ctx.upload(np.ascontiguousarray(wl, dtype=np.uint64))
    try:
        return ia.Whitelist(ctx, d, len(wl), bc_len)
    finally:
        d.free()


def _view(ia, ctx, buf, offset, nbytes):
    return ia.DeviceBuffer.wrap(ctx, buf.ptr + offset, max(nbytes, 1))


def _probe_codes(wl, bc_len):
    """What counts() is asked: every entry, neighbours of entries (mostly not in the whitelist), and below 32 bases an entry
    with a bit above 2*bc_len (not a code: 0)."""
    u = np.unique(wl)
    extra = [u[: 64] ^ np.uint64(1), u[: 64] ^ np.uint64(2 << (2 * (bc_len - 1)))]
    if bc_len < 32:
        extra.append(u[: 8] | np.uint64(1 << (2 * bc_len)))
    return np.concatenate([u] + extra)


@functools.lru_cache(maxsize=4)
def _case(bc_len, w):
    """The largest input of a (bc_len, w) cell with what correction leaves of it; the smaller sizes are prefixes (the mix is shuffled)."""
    rng = np.random.default_rng(0x1B00A00 + 1000 * bc_len + w % 997)
    wl, bc = rnp.make_case(rng, bc_len, w, max(NS))
    recs = rnp.records(rng, bc)
    want, cls, _ = wnp.correct_records(recs, wl, bc_len, 1)
    return wl, recs, want, cls


@pytest.mark.parametrize("bc_len,w,n", CASES)
def test_chain_matches_numpy(ia, ctx, bc_len, w, n):
    """correct -> add (class 0) -> resolve on raw records whose base is 8 but not 16 bytes aligned (one record is peeled), the
    class bytes 0, 1, 2 and 15 bytes behind a 16-byte boundary."""
    wl, recs, want, cls = _case(bc_len, w)
    recs, want, cls = recs[:n], want[:n], cls[:n]
    ab_np = rnp.add(rnp.Abundance(wl, bc_len), want, cls, 1)
    out_np, cls_np, tot_np = rnp.resolve(ab_np, want, cls, 39, 40)
    codes = _probe_codes(wl, bc_len)
    ar = _arena(ia, ctx, *([24 * n, n] * len(CLASS_SKEWS)))
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h:
            for skew in CLASS_SKEWS:
                d, d_cls = ar.carve(24 * n, 8), ar.carve(n, skew)
                d.upload(recs)
                ctx.correct_barcodes(h, d, n, 1, d_cls, counts=False)
                with h.abundance() as ab:
                    assert ab.device_bytes >= 8 * (h.n_distinct + 1)
                    ab.add(d, n, d_cls, 1)
                    tot = ctx.resolve_barcodes(h, ab, d, n, d_cls)
                    got_counts = ab.counts(codes)
                ar.check(f"chain n={n} class skew={skew}")
                assert tot == tot_np, skew
                assert (d_cls.download(np.uint8, n) == cls_np).all(), skew
                assert d.download(count=24 * n).tobytes() == out_np.tobytes(), skew
                assert (got_counts == rnp.counts(ab_np, codes)).all(), skew
    finally:
        ar.free()


def _set_counter(ctx, ab, code, count, bc_len, rng, chunk=100_000):
    """`count` reads of `code` into the abundance: add calls over one array of at most `chunk` records of that barcode."""
    if count == 0:
        return
    k = min(count, chunk)
    bc = wnp.with_junk(rng, np.full(k, code, np.uint64), bc_len)
    d = ctx.upload(rnp.records(rng, bc))
    left = count
    while left:
        step = min(left, k)
        ab.add(d, step)
        left -= step
    ctx.synchronize()
    d.free()


@pytest.mark.parametrize("num,den", rnp.SHARES)
@pytest.mark.parametrize("bc_len", [16, 32])
def test_share_boundary(ia, ctx, bc_len, num, den):
    """Counters set exactly: best * den == num * total resolves, one read fewer does not, total == 0 is `unseen`, three candidates."""
    wl, setc, mids, outcome, low = rnp.boundary_case(bc_len, num, den)
    rng = np.random.default_rng(3)
    ab_np = rnp.Abundance(wl, bc_len)
    for code, k in setc:
        ab_np.n[np.searchsorted(ab_np.wl, np.uint64(code))] += np.uint64(k)
    recs = rnp.records(rng, wnp.with_junk(rng, mids, bc_len))
    cls0 = np.full(len(mids), 2, np.uint8)
    out_np, cls_np, tot_np = rnp.resolve(ab_np, recs, cls0, num, den)
    assert (out_np["barcode"] & wnp.mask(bc_len) == low).all() if bc_len < 32 else (out_np["barcode"] == low).all()
    assert [k for k in rnp.TOTALS[1:] for _ in range(tot_np[k])] == sorted(outcome, key=rnp.TOTALS.index)
    with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
        for code, k in setc:
            _set_counter(ctx, ab, code, k, bc_len, rng)
        assert (ab.counts(ab_np.wl) == ab_np.n).all()
        n = len(mids)
        d, d_cls = ctx.upload(recs), ctx.alloc(16)
        assert ctx.correct_barcodes(h, d, n, 1, d_cls)["ambiguous"] == n
        tot = ctx.resolve_barcodes(h, ab, d, n, d_cls, (num, den))
        print(num, den, tot, [c for _, c in setc])
        assert tot == tot_np
        assert (d_cls.download(np.uint8, n) == cls_np).all() and d.download(wnp.REC, n).tobytes() == out_np.tobytes()
        d.free(); d_cls.free()


@pytest.mark.parametrize("bc_len", [16, 22, 23, 32])
def test_ballot_seam(ia, ctx, bc_len):
    """The winner and its rival in neighbours 0..63, on either side of 63 / 64, or both above; the winner first or second; at 32
    bases the all-ones key, whose counter lives outside the table, as winner and as loser."""
    wl, bc, low, mids = rnp.seam_case(bc_len)
    recs = rnp.records(np.random.default_rng(4), bc)
    out_np, cls_np, tot_np, ab_np = rnp.chain(wl, bc_len, recs)
    n = len(recs)
    with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
        d, d_cls = ctx.upload(recs), ctx.alloc(max(n, 16))
        ctx.correct_barcodes(h, d, n, 1, d_cls, counts=False)
        ab.add(d, n, d_cls, 1)
        tot = ctx.resolve_barcodes(h, ab, d, n, d_cls)
        got, got_cls = d.download(wnp.REC, n), d_cls.download(np.uint8, n)
        assert (ab.counts(ab_np.wl) == ab_np.n).all()
        d.free(); d_cls.free()
    assert tot == tot_np == {"examined": len(mids), "resolved": len(mids), "below_share": 0, "unseen": 0}
    assert (got_cls == cls_np).all() and got.tobytes() == out_np.tobytes()
    at = {int(b): k for k, b in enumerate(bc)}
    assert (got["barcode"][[at[int(c)] for c in mids]] == low).all()


def test_accumulation_and_masks(ia, ctx):
    """Two calls equal one over the concatenation; no class bytes against class_mask 0b0001, 0b0011 and 0; class bytes above 7 never
    count; reset; two streams adding to one abundance at once give the sum."""
    bc_len, n = 16, 100_003
    wl, recs, want, cls = _case(bc_len, 1000)
    recs, want, cls = recs[:n], want[:n], cls[:n].copy()
    rng = np.random.default_rng(5)
    odd = rng.random(n) < 0.1
    cls[odd] = rng.choice(np.array([4, 7, 8, 9, 200, 255], np.uint8), int(odd.sum()))    # 4 and 7 count under a mask that has their bit
    codes = np.unique(wl)
    half = 50_001                                                                       # an odd row: the second half peels a record
    other = ia.Context(0)                                                               # its stream is a second hardware queue on the same device
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
            d, d_cls, d_raw = ctx.upload(want), ctx.upload(cls), ctx.upload(recs)
            assert not ab.counts(codes).any()                                           # zero after create
            for mask in (None, 0b0001, 0b0011, 0, 0b10010000, 0xFFFFFFFF):
                ab.reset()
                ab.add(d, n, None if mask is None else d_cls, 1 if mask is None else mask)
                ref = rnp.add(rnp.Abundance(wl, bc_len), want, None if mask is None else cls, 1 if mask is None else mask)
                assert (ab.counts(codes) == ref.n).all(), mask
                assert mask != 0 or not ref.n.any()
            ab.reset()
            ab.add(d_raw, n)                                                            # raw records, no class bytes: the exact hits
            assert (ab.counts(codes) == rnp.add(rnp.Abundance(wl, bc_len), recs).n).all()
            assert int(ab.counts(codes).sum()) == int((wnp.correct_records(recs, wl, bc_len, 1)[1] == 0).sum())
            ab.reset()
            assert not ab.counts(codes).any()
            whole = rnp.add(rnp.Abundance(wl, bc_len), want, cls, 0b0011)
            parts = [(_view(ia, ctx, d, 0, 24 * half), half, _view(ia, ctx, d_cls, 0, half)),
                     (_view(ia, ctx, d, 24 * half, 24 * (n - half)), n - half, _view(ia, ctx, d_cls, half, n - half))]
            for p, k, c in parts:                                                       # one after the other
                ab.add(p, k, c, 0b0011)
            assert (ab.counts(codes) == whole.n).all()
            ab.add(d, n, d_cls, 0b0011)                                                 # and it keeps accumulating
            assert (ab.counts(codes) == 2 * whole.n).all()
            ab.reset()
            for (p, k, c), st in zip(parts, (None, other.stream)):                      # both at once
                ab.add(p, k, c, 0b0011, stream=st)
            ctx.synchronize()
            ctx.synchronize(other.stream)
            assert (ab.counts(codes) == whole.n).all()
            for b in (d, d_cls, d_raw):
                b.free()
    finally:
        other.close()


def _merge_inputs(wl, bc_len):
    """Grouped barcodes: sorted input; one barcode over whole tiles and across tile and lane seams; alternating pairs; runs of a
    barcode that is not in the whitelist between runs of one that is."""
    rng = np.random.default_rng(6)
    x, y, z = (np.uint64(v) for v in wl[:3])
    out_of = np.uint64(int(wl[3]) ^ 0b11 ^ (0b11 << 8))
    mixed = np.concatenate([wl[rng.integers(0, len(wl), 3000)], wnp.substitute(rng, wl[rng.integers(0, len(wl), 1000)], bc_len),
                            wnp.random_codes(rng, bc_len, 500)])
    runs = [(x, 300), (y, 1), (x, 129), (z, 127), (out_of, 130), (z, 2), (y, 255), (x, 1), (out_of, 1), (x, 128), (y, 128), (z, 3)]
    inputs = {"sorted": np.sort(mixed),
              "one barcode": np.full(1000, x, np.uint64),
              "runs": np.concatenate([np.full(k, v, np.uint64) for v, k in runs]),
              "alternating": np.tile(np.array([x, y], np.uint64), 700),
              "pairs": np.tile(np.array([x, x, y, y, out_of, out_of], np.uint64), 300),
              "offset pairs": np.concatenate([[z], np.tile(np.array([x, x, y, y], np.uint64), 300)])}
    return {k: wnp.with_junk(rng, v, bc_len) for k, v in inputs.items()}


@pytest.mark.parametrize("skew", [0, 8])
def test_run_merging(ia, ctx, skew):
    """Each grouped input gives the counters of its shuffled copy (and of numpy), with and without class bytes that switch records
    off in the middle of a run, on a 16-byte aligned base and on one that peels a record (every lane seam moves by one)."""
    bc_len = 16
    wl = _case(bc_len, 1000)[0]
    codes = np.unique(wl)
    rng = np.random.default_rng(7)
    with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
        for name, bc in _merge_inputs(wl, bc_len).items():
            n = len(bc)
            cls = rng.choice(np.array([0, 0, 0, 1, 3, 9], np.uint8), n)
            perm = rng.permutation(n)
            got = []
            ar = _arena(ia, ctx, 24 * n, n, 24 * n, n)
            try:
                for order in (np.arange(n), perm):
                    d, d_cls = ar.carve(24 * n, skew), ar.carve(n, 1)
                    d.upload(rnp.records(rng, bc[order]))
                    d_cls.upload(cls[order])
                    for c, mask in ((None, 1), (d_cls, 0b0001), (d_cls, 0b1010)):
                        ab.reset()
                        ab.add(d, n, c, mask)
                        got.append(ab.counts(codes))
                        ref = rnp.add(rnp.Abundance(wl, bc_len), bc, None if c is None else cls, mask)
                        assert (got[-1] == ref.n).all(), (name, mask)
                ar.check(f"add {name} skew={skew}")
            finally:
                ar.free()
            for a, b in zip(got[:3], got[3:]):
                assert (a == b).all(), name


def test_idempotence_and_untouched_data(ia, ctx):
    """A second resolve changes nothing; records of classes 0, 1, 3 and 4..255 are bit-identical afterwards, whatever their
    barcodes are; class 2 on a record that correction would not have called ambiguous is examined like any other; guard zones
    around records, class bytes, codes and counts are intact."""
    bc_len, n = 16, 100_003
    wl, recs, want, cls = _case(bc_len, 1000)
    want, cls = want[:n], cls[:n].copy()
    rng = np.random.default_rng(8)
    ab_np = rnp.add(rnp.Abundance(wl, bc_len), want, cls, 1)
    odd = rng.random(n) < 0.3
    cls[odd] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 7, 8, 200, 255], np.uint8), int(odd.sum()))
    out_np, cls_np, tot_np = rnp.resolve(ab_np, want, cls, 39, 40)
    assert tot_np["resolved"] > 0 and tot_np["examined"] > (cls[~odd] == 2).sum()
    codes = _probe_codes(wl, bc_len)
    k = len(codes)
    ar = _arena(ia, ctx, 24 * n, n, 8 * k, 8 * k)
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
            d, d_cls, d_codes, d_counts = ar.carve(24 * n, 8), ar.carve(n, 1), ar.carve(8 * k), ar.carve(8 * k)
            d.upload(want); d_cls.upload(cls); d_codes.upload(codes)
            ab.add(d, n, d_cls, 0)                                               # a mask of 0 adds nothing
            pure, pure_cls = ctx.upload(want), ctx.upload(_case(bc_len, 1000)[3][:n])
            ab.add(pure, n, pure_cls, 1)                                         # the exact reads, by the classes correction gave
            tot = ctx.resolve_barcodes(h, ab, d, n, d_cls)
            ia._check(ia.lib.ibu_abundance_counts(ctx._c, ab._c, d_codes.ptr, k, d_counts.ptr, None))
            ar.check("resolve and counts")
            assert tot == tot_np
            got, got_cls = d.download(count=24 * n).view(wnp.REC), d_cls.download(np.uint8, n)
            assert (got_cls == cls_np).all() and got.tobytes() == out_np.tobytes()
            assert (d_counts.download(np.uint64, k) == rnp.counts(ab_np, codes)).all()
            keep = cls != 2
            assert got[keep].tobytes() == want[keep].tobytes() and (got_cls[keep] == cls[keep]).all()
            assert (got["umi"] == want["umi"]).all() and (got["index"] == want["index"]).all()
            m = wnp.mask(bc_len)
            assert ((got["barcode"] & ~m) == (want["barcode"] & ~m)).all()
            again = ctx.resolve_barcodes(h, ab, d, n, d_cls)
            ar.check("second resolve")
            left = tot_np["examined"] - tot_np["resolved"]
            assert again == {"examined": left, "resolved": 0, "below_share": tot_np["below_share"], "unseen": tot_np["unseen"]}
            assert d.download(count=24 * n).tobytes() == out_np.tobytes() and (d_cls.download(np.uint8, n) == cls_np).all()
            assert ctx.resolve_barcodes(h, ab, d, n, d_cls, counts=False) is None   # asynchronous form
            ctx.synchronize()
            assert d.download(count=24 * n).tobytes() == out_np.tobytes() and (d_cls.download(np.uint8, n) == cls_np).all()
            assert (ab.counts(codes) == rnp.counts(ab_np, codes)).all()            # resolve adds nothing
            pure.free(); pure_cls.free()
    finally:
        ar.free()


def test_argument_errors(ia, ctx):
    bc_len, n = 16, 1000
    wl, recs, want, cls = _case(bc_len, 1000)
    lib = ia.lib

    def refused(rc):
        return rc != 0 and lib.ibu_status_name(rc) == b"InvalidArg"

    other = ia.Context(0)
    try:
        with _whitelist(ia, ctx, wl, bc_len) as h, _whitelist(ia, ctx, wl[:10], bc_len) as h2, _whitelist(ia, other, wl, bc_len) as h3:
            ab, ab3 = h.abundance(), h3.abundance()
            d, d_cls = ctx.upload(want[:n]), ctx.upload(cls[:n])
            before = (d.download().tobytes(), d_cls.download().tobytes())
            ok = (ctx._c, h._c, ab._c, d.ptr, n, 39, 40, d_cls.ptr, None, None)

            def resolve(**kw):
                names = ("ctx", "wl", "ab", "recs", "n", "num", "den", "cls", "counts", "stream")
                return lib.ibu_resolve_barcodes(*[kw.get(k, v) for k, v in zip(names, ok)])

            assert refused(resolve(wl=h2._c))                                    # the abundance belongs to another whitelist
            assert refused(resolve(wl=h3._c)) and refused(resolve(ab=ab3._c)) and refused(resolve(ctx=other._c))
            assert refused(resolve(wl=None)) and refused(resolve(ab=None)) and refused(resolve(ctx=None))
            for num, den in ((1, 2), (20, 40), (3, 2), (1 << 24, 1 << 24), ((1 << 23) + 1, 1 << 24), (0, 0), (1, 0), (0, 1)):
                assert refused(resolve(num=num, den=den)), (num, den)
                assert refused(resolve(num=num, den=den, n=0)), (num, den)         # checked whatever n is
            assert refused(resolve(cls=None)) and refused(resolve(recs=None)) and refused(resolve(recs=d.ptr + 4))
            assert refused(resolve(n=1 << 40))
            c = ia._lib.CResolveCounts(9, 9, 9, 9)
            assert resolve(n=0, counts=C.byref(c)) == 0 and (c.examined, c.resolved, c.below_share, c.unseen) == (0, 0, 0, 0)
            assert resolve(n=0, recs=None, cls=None) == 0
            assert ctx.resolve_barcodes(h, ab, d, 0, d_cls) == dict.fromkeys(rnp.TOTALS, 0)
            # add and counts
            assert refused(lib.ibu_abundance_add(other._c, ab._c, d.ptr, None, n, 1, None))
            assert refused(lib.ibu_abundance_add(ctx._c, ab3._c, d.ptr, None, n, 1, None))
            assert refused(lib.ibu_abundance_add(ctx._c, None, d.ptr, None, n, 1, None))
            assert refused(lib.ibu_abundance_add(ctx._c, ab._c, None, None, n, 1, None))
            assert refused(lib.ibu_abundance_add(ctx._c, ab._c, d.ptr, None, 1 << 40, 1, None))
            assert lib.ibu_abundance_add(ctx._c, ab._c, None, None, 0, 1, None) == 0
            assert refused(lib.ibu_abundance_counts(ctx._c, ab3._c, d.ptr, 1, d.ptr, None))
            assert refused(lib.ibu_abundance_counts(ctx._c, ab._c, None, 1, d.ptr, None))
            assert lib.ibu_abundance_counts(ctx._c, ab._c, None, 0, None, None) == 0
            h4 = C.c_void_p()
            assert refused(lib.ibu_abundance_create(ctx._c, h3._c, None, C.byref(h4))) and not h4.value
            assert refused(lib.ibu_abundance_create(ctx._c, None, None, C.byref(h4)))
            ctx.synchronize()
            assert not ab.counts(np.unique(wl)).any(), "a refused call adds nothing"
            assert (d.download().tobytes(), d_cls.download().tobytes()) == before, "a refused call touches nothing"
            # the running total of records offered: 100 so far, 2^40 - 50 more would pass 2^40 — refused before anything is launched
            ab.add(d, 100)
            rc = lib.ibu_abundance_add(ctx._c, ab._c, d.ptr, None, (1 << 40) - 50, 1, None)
            assert refused(rc)
            det = ia.CErrorDetail()
            lib.ibu_last_error(C.byref(det))
            assert (det.a, det.b) == (100, (1 << 40) - 50)
            ctx.synchronize()
            assert int(ab.counts(np.unique(wl)).sum()) == int(np.isin(want["barcode"][:100] & wnp.mask(bc_len), wl).sum()) > 0
            ab.reset()
            ab.add(d, 100)                                                         # reset starts the total again
            ab.close(); ab3.close()
            ab.close()                                                             # twice is harmless
            d.free(); d_cls.free()
    finally:
        other.close()


def _numpy_pipeline(recs, wl, bc_len, keep, num=39, den=40):
    out, cls, tot, _ = rnp.chain(wl, bc_len, recs, num, den)
    kept = out[np.isin(cls, keep)]
    kept = kept[np.lexsort((kept["index"], kept["umi"], kept["barcode"]))]
    b, c = np.unique(kept["barcode"], return_counts=True)
    return kept, b, c.astype(np.uint64), tot


def test_the_chain_the_feature_exists_for(ia, ctx):
    """correct -> add (class 0) -> resolve -> select exact | corrected | resolved -> sort -> per-barcode counts equals the same in
    numpy, and keeps strictly more records than exact | corrected does."""
    bc_len, n = 16, 100_003
    wl, recs, _, _ = _case(bc_len, 1000)
    recs = recs[:n].copy()
    recs["barcode"] &= wnp.mask(bc_len)
    kept, want_b, want_c, tot = _numpy_pipeline(recs, wl, bc_len, (0, 1, 4))
    fewer = _numpy_pipeline(recs, wl, bc_len, (0, 1))[0]
    assert tot["resolved"] > 0 and len(kept) == len(fewer) + tot["resolved"]
    d, tmp, d_cls = ctx.upload(recs), ctx.alloc(24 * n), ctx.alloc(n)
    with _whitelist(ia, ctx, wl, bc_len) as h, h.abundance() as ab:
        ctx.correct_barcodes(h, d, n, 1, d_cls, counts=False)
        ab.add(d, n, d_cls, 1 << 0)
        assert ctx.resolve_barcodes(h, ab, d, n, d_cls) == tot
    out2, k2 = ctx.select_records(d, d_cls, n, 0b0011)
    out, k = ctx.select_records(d, d_cls, n, 0b10011)
    assert k == len(kept) and k2 == len(fewer) and k > k2
    ctx.sort_records(out, tmp, k)
    assert out.download(wnp.REC, k).tobytes() == kept.tobytes()
    got_b, got_c, _ = ctx.barcode_counts(out, k, unique_umis=False)
    assert (got_b == want_b).all() and (got_c == want_c).all() and len(got_b) <= len(np.unique(wl))
    for b in (d, tmp, d_cls, out, out2):
        b.free()


def test_correct_file_example_resolves(ia, tmp_path):
    from ibu_amd import _lib
    exe = tmp_path / "correct_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "correct_file.cpp"),
                           "-o", str(exe), _lib.SO_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len, n = 16, 50_000
    rng = np.random.default_rng(0x1B00A01)
    wl, bc = rnp.make_case(rng, bc_len, 2000, n, junk=False)
    recs = rnp.records(rng, bc)
    recs["umi"] &= wnp.mask(12)
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), ia.Header(bc_len, 12))
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    text = ["".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(bc_len)) for c in wl]   # base i at bits [2i, 2i+1]
    (tmp_path / "wl.txt").write_text("\n".join(text) + "\n")
    for flag, share in (("--resolve", (39, 40)), ("--resolve=3/4", (3, 4))):
        r = subprocess.run([str(exe), str(tmp_path / "in.ibu"), str(tmp_path / "wl.txt"), str(tmp_path / "out.ibu"), flag],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        kept, want_b, _, tot = _numpy_pipeline(recs, wl, bc_len, (0, 1, 4), *share)
        assert tot["resolved"] > 0
        h, got = ia.load_to_vec(str(tmp_path / "out.ibu"))
        assert h.sorted() and np.asarray(got).tobytes() == kept.tobytes()
        assert (f"ambiguous examined {tot['examined']}: resolved {tot['resolved']} at a share of {share[0]}/{share[1]}, below the share "
                f"{tot['below_share']}, no exact read among the candidates {tot['unseen']}") in r.stdout
        assert f"kept {len(kept)}" in r.stdout and f"after {len(want_b)}" in r.stdout
    r = subprocess.run([str(exe), str(tmp_path / "in.ibu"), str(tmp_path / "wl.txt"), str(tmp_path / "out.ibu"), "--resolve=1/2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "2 * num > den" in r.stderr
