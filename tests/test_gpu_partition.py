"""ibu_partition_records on the device against tests/partition_np.py, byte for byte: every size, part count and class pattern at
which the count, the scan or the scatter can go wrong, in guard arenas at contract size; the refusals; partition_by_label; the
demux_file example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import count_np as cnp
from tests import label_np as lnp
from tests import partition_np as pnp
from tests.test_gpu_resolve import PATTERN, Arena, _arena, _whitelist  # noqa: F401
from tests.test_gpu_sweeps import _context, cus  # noqa: F401  (cus: a fixture, on this module's ia and ctx)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = [1, 2, 3, 16, 64, 65, 255]
U = pnp.unit_of(max(PARTS))                                      # 16384: the unit of the most parts
SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17, U - 1, U, U + 1, 2 * U + 5, 100_003]
SCAN_STEP = 16384                                                # kcommon.hpp: kScanBlock * kScanPer entries per iteration of the scan


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
def pool():
    """The records every case takes a prefix of: random words, the index column the input position."""
    n = 100_003
    rng = np.random.default_rng(0x9A7717)
    recs = np.zeros(n, cnp.REC)
    recs["barcode"] = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    recs["umi"] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    recs["index"] = np.arange(n, dtype=np.uint64)
    recs.setflags(write=False)
    return recs


def _p(buf):
    return C.c_void_p(buf.ptr) if buf is not None else None


def _call(ia, ctx, d, d_cls, n, part_of, n_parts, d_out, cap, offsets="own"):
    """The C call -> (rc, offsets as numpy).  offsets: "own" = n_parts + 1 words preset to a marker, or None."""
    off = None
    if offsets == "own":
        off = (C.c_uint64 * (min(max(n_parts, 0), 255) + 1))(*([0xDEAD] * (min(max(n_parts, 0), 255) + 1)))
    po = None if part_of is None else np.ascontiguousarray(part_of, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    rc = ia.lib.ibu_partition_records(ctx._c, _p(d), _p(d_cls), n, po, n_parts, _p(d_out), cap, off, None)
    return rc, (None if off is None else np.array(off, dtype=np.uint64))


def crafted(n_parts):
    """Non-injective, every fifth class dropped, class 255 mapped to a part.  7 is coprime to every part count used, so the classes
    0 .. n_parts + 1 that are not dropped go to distinct parts: four parts in five are reached."""
    c = np.arange(256)
    m = ((c * 7 + 3) % n_parts).astype(np.uint8)
    m[c % 5 == 1] = pnp.NONE
    m[255] = n_parts - 1
    assert pnp.check_map(m, n_parts)
    return m


def _kept_classes(pmap, n_parts):
    """One class per part where there is one (the lowest), in part order."""
    return np.array([np.flatnonzero(pmap == p)[0] for p in range(n_parts) if (pmap == p).any()], np.uint8)


def patterns(rng, n, n_parts, pmap):
    """{name: class bytes}.  `pmap`: the full 256-entry map in force (the identity spelled out)."""
    i = np.arange(n)
    unit = pnp.unit_of(n_parts)
    dropped = np.uint8(np.flatnonzero(pmap == pnp.NONE)[0])
    kept = _kept_classes(pmap, n_parts)
    out = {}
    uniform = rng.integers(0, min(n_parts + 2, 256), n).astype(np.uint8)
    uniform[rng.random(n) < 0.03] = 255
    out["uniform"] = uniform
    out["one_class"] = np.full(n, kept[-1], np.uint8)            # every lane a peer: the leader adds 64
    out["modulo"] = (i % n_parts).astype(np.uint8)               # from 64 parts on every lane of a round is alone in its part
    cuts = sorted({k * unit + d for k in range(1, n // unit + 2) for d in (-1, 0, 1) if 0 < k * unit + d < n} | ({n // 2} if n > 1 else set()))
    run = np.searchsorted(np.array(cuts, np.int64), i, side="right") if cuts else np.zeros(n, np.int64)
    out["runs"] = (run % min(n_parts + 1, 256)).astype(np.uint8)  # long runs that end at the unit seams and one record either side
    out["all_dropped"] = np.full(n, dropped, np.uint8)
    out["alternating"] = np.where(i % 2 == 0, kept[(i // 2) % len(kept)], dropped).astype(np.uint8)
    single = np.full(n, dropped, np.uint8)
    if n:
        single[n - 1] = kept[0]                                  # one kept record in the last round of the ragged tail
    out["single_last"] = single
    return out


def _run_case(ia, ctx, ar, d, d_cls, d_out, recs, cls, part_of, n_parts, cap, what):
    n = len(recs)
    want, want_off, _ = pnp.partition(recs, cls, part_of, n_parts)
    if n:
        d_cls.upload(cls)
    if cap:
        d_out.upload(np.full(24 * cap, PATTERN, np.uint8))
    rc, off = _call(ia, ctx, d, d_cls, n, part_of, n_parts, d_out, cap)
    assert rc == 0, (what, rc)
    ar.check(what)
    assert off.tobytes() == want_off.tobytes(), (what, off, want_off)
    got = d_out.download(count=24 * cap) if cap else np.empty(0, np.uint8)
    k = len(want)
    assert got[:24 * k].tobytes() == want.tobytes(), what
    assert (got[24 * k:] == PATTERN).all(), f"{what}: bytes behind the last kept record were written"
    return want, want_off


@pytest.mark.parametrize("skew", [0, 8])
@pytest.mark.parametrize("n_parts", PARTS)
def test_partition_matches_numpy(ia, ctx, pool, n_parts, skew):
    """Every size x class pattern x map.  skew 8: d_records and d_out 8 but not 16 bytes behind a 256-byte boundary, the class
    pointer odd.  d_out holds n records: whatever is not kept leaves the bytes behind the last kept record untouched."""
    rng = np.random.default_rng(0x9A77 + 1000 * n_parts + skew)
    unit = pnp.unit_of(n_parts)
    sizes = sorted(set(SIZES) | {unit - 1, unit, unit + 1})
    for n in sizes:
        recs = pool[:n]
        ar = _arena(ia, ctx, 24 * n, n, 24 * n)
        try:
            d, d_cls, d_out = ar.carve(24 * n, skew), ar.carve(n, 1 if skew else 0), ar.carve(24 * n, skew)
            if n:
                d.upload(recs)
            for map_name, part_of in (("identity", None), ("crafted", crafted(n_parts))):
                pmap = pnp.identity(n_parts) if part_of is None else part_of
                for name, cls in patterns(rng, n, n_parts, pmap).items():
                    _run_case(ia, ctx, ar, d, d_cls, d_out, recs, cls, part_of, n_parts, n, f"n_parts={n_parts} n={n} {map_name} {name}")
            if n:
                assert d.download(count=24 * n).tobytes() == recs.tobytes()          # the input is never written
        finally:
            ar.free()


def test_the_patterns_reach_what_they_are_for():
    """The cases above, looked at on the host: lanes alone in their part, whole rounds of one part, run ends at unit seams +- 1,
    a single kept record in a ragged last round."""
    rng = np.random.default_rng(1)
    for n_parts in PARTS:
        unit = pnp.unit_of(n_parts)
        n = 2 * U + 5
        pm = pnp.identity(n_parts)
        pt = patterns(rng, n, n_parts, pm)
        part = pm[pt["modulo"]][:64]
        assert len(set(part.tolist())) == min(n_parts, 64)
        assert len(set(pm[pt["one_class"]].tolist())) == 1 and pm[pt["one_class"][0]] != pnp.NONE
        ends = np.flatnonzero(pt["runs"][1:] != pt["runs"][:-1]) + 1
        assert {unit - 1, unit, unit + 1} <= set(ends.tolist())
        assert (pm[pt["all_dropped"]] == pnp.NONE).all()
        alt = pm[pt["alternating"]]
        assert (alt[1::2] == pnp.NONE).all() and (alt[0::2] != pnp.NONE).all()
        s = pm[pt["single_last"]]
        assert (s != pnp.NONE).sum() == 1 and s[-1] != pnp.NONE and n % 64 != 0
        cm = crafted(n_parts)
        live = cm[cm != pnp.NONE]
        assert cm[255] != pnp.NONE and (cm == pnp.NONE).any() and len(set(live.tolist())) < len(live)   # non-injective, with drops
        used = cm[np.arange(min(n_parts + 2, 256))]                # the classes the patterns draw from reach most parts (the identity: all)
        assert len(set(used[used != pnp.NONE].tolist())) >= max(n_parts * 3 // 4, 1)


def test_capacity_larger_than_the_total(ia, ctx, pool):
    """cap between the records kept and n, and cap above n: the bytes behind the last kept record stay as they were."""
    n, n_parts = 3 * 2048 + 17, 3
    rng = np.random.default_rng(7)
    cls = rng.integers(0, 6, n).astype(np.uint8)                 # identity: about half are kept
    kept = int((cls < n_parts).sum())
    for cap in (kept, kept + 1, n + 100):
        ar = _arena(ia, ctx, 24 * n, n, 24 * cap)
        try:
            d, d_cls, d_out = ar.carve(24 * n), ar.carve(n), ar.carve(24 * cap)
            d.upload(pool[:n])
            _run_case(ia, ctx, ar, d, d_cls, d_out, pool[:n], cls, None, n_parts, cap, f"cap={cap} kept={kept}")
        finally:
            ar.free()


def test_scan_seams(ia, ctx):
    """A flattened table longer than one iteration of the scan (16384 entries): 17 parts over 1024 units of 2048 records, so the
    start of part 16 is entry 16384, exactly on the seam, and every other part start lies inside an iteration.  Few records are kept:
    the output stays small."""
    n_parts, nunits = 17, 1024
    assert pnp.unit_of(n_parts) == 2048 and n_parts * nunits > SCAN_STEP and 16 * nunits == SCAN_STEP
    n = (nunits - 1) * 2048 + 77
    rng = np.random.default_rng(0x5CA9)
    recs = np.zeros(n, cnp.REC)
    recs["barcode"], recs["umi"], recs["index"] = rng.integers(0, 1 << 62, n, dtype=np.uint64), 7, np.arange(n, dtype=np.uint64)
    cls = np.where(rng.random(n) < 0.08, rng.integers(0, n_parts, n), 200).astype(np.uint8)
    cls[(np.arange(n) // 2048) % 5 == 2] = 200                   # whole units that keep nothing
    want, want_off, _ = pnp.partition(recs, cls, None, n_parts)
    assert (np.diff(want_off.astype(np.int64)) > 0).all()
    cap = len(want)
    ar = _arena(ia, ctx, 24 * n, n, 24 * cap)
    try:
        d, d_cls, d_out = ar.carve(24 * n), ar.carve(n), ar.carve(24 * cap)
        d.upload(recs)
        _run_case(ia, ctx, ar, d, d_cls, d_out, recs, cls, None, n_parts, cap, "scan seams")
    finally:
        ar.free()


def test_waves_that_sweep_three_units(ia, cus):  # noqa: F811
    """One workgroup per CU: every wave sweeps at least three units and some four, so a wave's positions per part must be loaded
    again for every unit, and its counters cleared."""
    c = _context(ia)
    try:
        n_parts = 5
        nunits = 3 * 4 * cus + 5
        n = (nunits - 1) * 2048 + 77
        rng = np.random.default_rng(0x3A11)
        recs = np.zeros(n, cnp.REC)
        recs["barcode"], recs["umi"], recs["index"] = rng.integers(0, 1 << 62, n, dtype=np.uint64), 3, np.arange(n, dtype=np.uint64)
        unit = np.arange(n) // 2048
        cls = np.where(unit % 3 == 0, 9, np.where(unit % 3 == 1, 4, rng.integers(0, 12, n))).astype(np.uint8)
        cls[rng.random(n) < 0.7] = 9                             # most are dropped: the output stays small
        part_of = pnp.identity(n_parts)
        part_of[11] = 0
        want, want_off, _ = pnp.partition(recs, cls, part_of, n_parts)
        cap = len(want)
        ar = _arena(ia, c, 24 * n, n, 24 * cap)
        try:
            d, d_cls, d_out = ar.carve(24 * n), ar.carve(n), ar.carve(24 * cap)
            d.upload(recs)
            _run_case(ia, c, ar, d, d_cls, d_out, recs, cls, part_of, n_parts, cap, "three units per wave")
        finally:
            ar.free()
    finally:
        c.close()


def test_parts_of_sorted_records_are_sorted(ia, ctx):
    """sort_records, classes that depend on the barcode only, partition: every part passes the sorted check and pair_counts on it
    equals numpy's on the numpy part — no second sort."""
    n, n_parts = 40_003, 6
    rng = np.random.default_rng(0x57AB1E)
    recs = cnp.make_records(rng, n, 16, 700, 40, 50)
    d, tmp = ctx.upload(recs), ctx.alloc(24 * n)
    d_cls = out = None
    try:
        ctx.sort_records(d, tmp, n)
        srt = d.download(cnp.REC, n)
        assert srt.tobytes() == cnp.sort_records(recs).tobytes()
        cls = (srt["barcode"] % np.uint64(8)).astype(np.uint8)   # classes 6 and 7 are dropped
        d_cls = ctx.upload(cls)
        out, off = ctx.partition_records(d, d_cls, n, n_parts=n_parts)
        want, want_off, _ = pnp.partition(srt, cls, None, n_parts)
        assert off.tobytes() == want_off.tobytes() and (np.diff(off.astype(np.int64)) > 0).all()
        assert out.download(cnp.REC, len(want)).tobytes() == want.tobytes()
        for p in range(n_parts):
            lo, k = int(off[p]), int(off[p + 1] - off[p])
            view = ia.DeviceBuffer.wrap(ctx, out.ptr + 24 * lo, 24 * k)
            assert ctx.is_sorted(view, k), p
            got = ctx.pair_counts(view, k)
            for g, w in zip(got, cnp.pair_counts(want[lo:lo + k])):
                assert np.asarray(g).tobytes() == w.tobytes(), p
    finally:
        for x in (d, tmp, d_cls, out):
            if x is not None:
                x.free()


# ---- refusals: each one touches nothing -------------------------------------------------------------------------------------------
@pytest.fixture()
def small(ia, ctx, pool):
    n = 5000
    cls = (np.arange(n) % 7).astype(np.uint8)
    ar = _arena(ia, ctx, 24 * n + 64, n, 24 * n + 64)
    d, d_cls, d_out = ar.carve(24 * n + 64), ar.carve(n), ar.carve(24 * n + 64)
    d.upload(np.concatenate([pool[:n].view(np.uint8), np.full(64, PATTERN, np.uint8)]))
    d_cls.upload(cls)
    d_out.upload(np.full(24 * n + 64, PATTERN, np.uint8))
    yield ar, d, d_cls, d_out, n, cls

    ar.free()


def _untouched(ia, ctx, small, pool, what):
    ar, d, d_cls, d_out, n, cls = small
    ar.check(what)
    assert (d_out.download(count=24 * n + 64) == PATTERN).all(), what
    assert d.download(count=24 * n).tobytes() == pool[:n].tobytes() and d_cls.download(count=n).tobytes() == cls.tobytes(), what


def _detail(ia):
    d = ia.CErrorDetail()
    ia.lib.ibu_last_error(C.byref(d))
    return d


def _refused(ia, rc, text):
    assert rc != 0 and ia.lib.ibu_status_name(rc) == b"InvalidArg", rc
    assert text in _detail(ia).message.decode(), _detail(ia).message


def test_refuses_part_of_entry_out_of_range(ia, ctx, small, pool):
    ar, d, d_cls, d_out, n, cls = small
    m = pnp.identity(4)
    m[77] = 4                                                    # neither below n_parts nor 255
    rc, off = _call(ia, ctx, d, d_cls, n, m, 4, d_out, n)
    _refused(ia, rc, "part_of[77] = 4")
    assert (off == 0xDEAD).all()
    _untouched(ia, ctx, small, pool, "part_of entry")


@pytest.mark.parametrize("n_parts", [0, 256])
def test_refuses_n_parts_out_of_range(ia, ctx, small, pool, n_parts):
    ar, d, d_cls, d_out, n, cls = small
    rc, off = _call(ia, ctx, d, d_cls, n, None, n_parts, d_out, n)
    _refused(ia, rc, "n_parts must be in 1 .. 255")
    assert (off == 0xDEAD).all()
    _untouched(ia, ctx, small, pool, f"n_parts={n_parts}")


def test_refuses_null_offsets(ia, ctx, small, pool):
    ar, d, d_cls, d_out, n, cls = small
    rc, _ = _call(ia, ctx, d, d_cls, n, None, 4, d_out, n, offsets=None)
    _refused(ia, rc, "offsets is NULL")
    _untouched(ia, ctx, small, pool, "offsets NULL")


@pytest.mark.parametrize("which", ["d_records", "d_out"])
def test_refuses_misaligned_pointers(ia, ctx, small, pool, which):
    ar, d, d_cls, d_out, n, cls = small
    off4 = lambda b: ia.DeviceBuffer.wrap(ctx, b.ptr + 4, 24 * (n - 1))   # noqa: E731
    rc, _ = _call(ia, ctx, off4(d) if which == "d_records" else d, d_cls, n - 1, None, 4, off4(d_out) if which == "d_out" else d_out, n - 1)
    _refused(ia, rc, f"{which} must be non-NULL and 8-byte aligned")
    _untouched(ia, ctx, small, pool, which)


def test_refuses_overlap(ia, ctx, small, pool):
    ar, d, d_cls, d_out, n, cls = small
    inside = ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * 100, 24 * 10)
    for out, cap, what in ((d, n, "the same array"), (inside, 10, "inside the records"), (inside, 0, "empty, inside the records")):
        rc, _ = _call(ia, ctx, d, d_cls, n, None, 4, out, cap)
        _refused(ia, rc, "d_out overlaps d_records")
        _untouched(ia, ctx, small, pool, what)
    behind = ia.DeviceBuffer.wrap(ctx, d.ptr + 24 * n, 48)       # the 64 spare bytes behind the records: no overlap
    rc, off = _call(ia, ctx, d, d_cls, 2, None, 1, behind, 2)
    assert rc == 0 and off.tolist() == [0, 1]


def test_cap_too_small_fills_offsets_and_writes_nothing(ia, ctx, small, pool):
    ar, d, d_cls, d_out, n, cls = small
    want, want_off, _ = pnp.partition(pool[:n], cls, None, 4)
    rc, off = _call(ia, ctx, d, d_cls, n, None, 4, d_out, len(want) - 1)
    _refused(ia, rc, "output capacity")
    det = _detail(ia)
    assert (det.a, det.b) == (len(want), len(want) - 1)
    assert off.tobytes() == want_off.tobytes()
    _untouched(ia, ctx, small, pool, "cap too small")


def test_size_query_and_empty_input(ia, ctx, small, pool):
    ar, d, d_cls, d_out, n, cls = small
    m = crafted(9)
    want, want_off, _ = pnp.partition(pool[:n], cls, m, 9)
    rc, off = _call(ia, ctx, d, d_cls, n, m, 9, None, 0)
    assert rc == 0 and off.tobytes() == want_off.tobytes()
    _untouched(ia, ctx, small, pool, "size query")
    rc, off = _call(ia, ctx, None, None, 0, None, 3, None, 0)    # n == 0: nothing is looked at
    assert rc == 0 and off.tolist() == [0, 0, 0, 0]
    _untouched(ia, ctx, small, pool, "n == 0")


# ---- the layers above -------------------------------------------------------------------------------------------------------------
def test_partition_by_label(ia, ctx):
    """Against label_np + partition_np: labels past 7 arrive (select_records could not keep them), barcodes that are no entry and
    entries with other labels are dropped."""
    bc_len, w, n = 16, 1000, 30_011
    labels = [0, 7, 8, 200, 254]
    rng = np.random.default_rng(0x1AB0700)
    wl = lnp.whitelist(rng, bc_len, w)
    lab = np.array([0, 7, 8, 200, 254, 3, 255][:7], np.uint8)[np.arange(w) % 7]   # labels 3 and 255 are on entries, and asked for by nobody
    recs = lnp.records(rng, lnp.barcodes(rng, wl, bc_len, n, miss=0.15))
    lb_np = lnp.Labels(wl, bc_len)
    assert lnp.set_labels(lb_np, wl, lab) == 0
    missing = 1                                                  # the lowest byte that is no label asked for
    cls_np, hist = lnp.label_records(lb_np, recs, missing_class=missing)
    assert hist[256] > 0 and all(hist[v] > 0 for v in labels + [3, 255])
    part_of = np.full(256, pnp.NONE, np.uint8)
    part_of[labels] = np.arange(len(labels))
    want, want_off, _ = pnp.partition(recs, cls_np, part_of, len(labels))
    assert [int(want_off[j + 1] - want_off[j]) for j in range(len(labels))] == [int(hist[v]) for v in labels]
    whitelist = _whitelist(ia, ctx, wl, bc_len)
    d = ctx.upload(recs)
    lb = out = None
    try:
        lb = whitelist.labels(fill=255)
        assert lb.set(wl, lab) == 0
        out, off = ctx.partition_by_label(lb, d, n, labels)
        assert off.tobytes() == want_off.tobytes()
        assert out.download(cnp.REC, len(want)).tobytes() == want.tobytes()
        for bad in ([], [1, 2, 1], list(range(256)), [256]):
            with pytest.raises(ValueError):
                ctx.partition_by_label(lb, d, n, bad)
    finally:
        for x in (out, d):
            if x is not None:
                x.free()
        if lb is not None:
            lb.close()
        whitelist.close()


def _text(code, bc_len):
    return "".join("ACGT"[(int(code) >> (2 * i)) & 3] for i in range(bc_len))   # base i at bits [2i, 2i+1]


def test_demux_file_example(ia, tmp_path):
    """demux_file --missing on a 5121-record file with three labels: the four files' records are the numpy parts, their headers the
    input's, and the #label lines the histogram."""
    from ibu_amd import _lib
    exe = tmp_path / "demux_file"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "demux_file.cpp"), "-o", str(exe), _lib.SO_PATH,
                           f"-Wl,-rpath,{os.path.dirname(_lib.SO_PATH)}", "-lpthread"])
    bc_len, n = 16, 5121
    rng = np.random.default_rng(0x1AB0800)
    cells = lnp.whitelist(rng, bc_len, 60)
    labs = np.array([2, 9, 200], np.uint8)[np.arange(60) % 3]
    recs = np.zeros(n, cnp.REC)
    recs["barcode"] = np.concatenate([cells[rng.integers(0, 60, n - 500)], lnp.outsiders(rng, cells, bc_len, 500)])[rng.permutation(n)]
    recs["umi"], recs["index"] = rng.integers(0, 40, n, dtype=np.uint64), rng.integers(0, 30, n, dtype=np.uint64)
    recs = cnp.sort_records(recs)                                # sorted input: the flag carries over and every part is sorted
    hdr = ia.Header(bc_len, 12)
    hdr.set_sorted()
    wr = ia.Writer.from_path(str(tmp_path / "in.ibu"), hdr)
    wr.write_batch(recs)
    wr.finish()
    wr.close()
    (tmp_path / "labels.txt").write_text("".join(f"{_text(c, bc_len)} {int(v)}\n" for c, v in zip(cells, labs)))
    lb_np = lnp.Labels(cells, bc_len)
    lnp.set_labels(lb_np, cells, labs)
    cls_np, hist = lnp.label_records(lb_np, recs)
    found = lnp.label_records(lb_np, recs, match=2)[0] != lnp.MISSING
    prefix = str(tmp_path / "out")
    r = subprocess.run([str(exe), "--missing", str(tmp_path / "in.ibu"), str(tmp_path / "labels.txt"), prefix], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    in_header = open(tmp_path / "in.ibu", "rb").read()[:32]
    parts = {"2": recs[found & (cls_np == 2)], "9": recs[found & (cls_np == 9)], "200": recs[found & (cls_np == 200)], "missing": recs[~found]}
    assert sum(len(v) for v in parts.values()) == n and len(parts["missing"]) == 500
    for name, want in parts.items():
        raw = open(f"{prefix}.{name}.ibu", "rb").read()
        assert raw[:32] == in_header, name
        assert raw[32:] == want.tobytes(), name
    assert sorted(os.listdir(tmp_path)) == sorted(["demux_file", "in.ibu", "labels.txt"] + [f"out.{k}.ibu" for k in parts])
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("#label")] == \
        [f"#label\t{k}\t{int(hist[k])}" for k in (2, 9, 200)] + [f"#label\t-\t{int(hist[256])}"]
