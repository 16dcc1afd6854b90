#!/usr/bin/env python3
"""Per-barcode aggregation (BarcodeAnalyzer, parallel.rs:72-98) on device-resident SORTED records: ibu_barcode_counts
timed by phase — the size query (count pass + scan + 16-byte read-back) and the emit call (count + scan + emit + finish)
into preallocated device arrays, no download.
  python tools/aggbench.py [--records 1e9] [--lens 10,12] [--rounds 5]
  python tools/aggbench.py --matrix 1e5x100,own_pair,one_pair [--records 1e9]     the count-matrix legs (matrix_legs below)
  python tools/aggbench.py --molecules [--records 1e9] [--reads-per-molecule 4] [--second-candidate 0.05]     ibu_classify_molecules (molecule_legs below)
  python tools/aggbench.py --cells [--records 1e9] [--reads-per-molecule 4]     ibu_call_cells (cell_legs below)
  python tools/aggbench.py --saturation [--records 1e9] [--reads-per-molecule 4]     ibu_saturation_curve, ibu_subsample_class (saturation_legs below)
  python tools/aggbench.py --metrics [--records 1e9] [--reads-per-molecule 4]     ibu_barcode_metrics, ibu_filter_barcodes (metrics_legs below)
  python tools/aggbench.py --features [--records 1e9] [--reads-per-molecule 4]     ibu_feature_metrics, ibu_filter_features (feature_legs below)
  python tools/aggbench.py --mtx [--records 1e8] [--host-entries 1e7]     ibu_matrix_rows, ibu_matrix_market_body (mtx_legs below; --records counts entries)
  python tools/aggbench.py --rowtop [--records 1e8]     ibu_matrix_row_top, ibu_assign_rows on the same entry table (rowtop_legs below)
bc_len 10 gives 2^20 distinct barcodes (a single-cell whitelist's order of magnitude); 16 gives ~n runs of length one."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rand_bits(torch, g, nbits, count):
    """count random nbits-bit values as int64 bit patterns (nbits up to 64)."""
    if nbits <= 62:
        return torch.randint(0, 1 << nbits, (count,), generator=g, device="cuda", dtype=torch.int64)
    hi = torch.randint(0, 1 << (nbits - 32), (count,), generator=g, device="cuda", dtype=torch.int64)
    return (hi << 32) | torch.randint(0, 1 << 32, (count,), generator=g, device="cuda", dtype=torch.int64)


def matrix_legs(a):
    """--matrix: the count-matrix path on resident 16/12 records, timed with events on a side stream (the first round is the
    warm-up).  Per input: ibu_records_swap_umi_index (out of place and in place) against ibu_device_copy of the same bytes on the
    same arrays; ibu_pair_counts (size query, and with outputs) against ibu_reduce (one plain read) and against
    ibu_barcode_counts with outputs on records that are each their own barcode (two reads and per-run outputs); ibu_count_matrix
    in one call and as its four steps."""
    import numpy as np
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    bc_len, umi_len = 16, 12
    orig, d, t = ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(24 * n)
    outs = [ctx.alloc(8 * n) for _ in range(4)]
    g = torch.Generator(device="cuda").manual_seed(0x1B00009)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stat(v):
        v = v[1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    def rounds(fn, before=None):
        v = []
        for _ in range(a.rounds + 1):
            if before:
                before()
                torch.cuda.synchronize()
            v.append(timed(fn))
        return stat(v)

    def restore():
        _check(lib.ibu_device_copy(ctx._c, _dptr(d), _dptr(orig), 24 * n, st))

    npairs, ntriples, nb, nbu = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    # the yardstick of the pair level: every record its own barcode, ibu_barcode_counts with outputs
    ctx.generate(0x1B00005, 0, n, bc_len, umi_len, d)
    ctx.sort_records(d, t, n)
    ctx.synchronize()
    own = rounds(lambda: _check(lib.ibu_barcode_counts(ctx._c, _dptr(d), n, _dptr(outs[0]), _dptr(outs[1]), _dptr(outs[2]), n, C.byref(nb), C.byref(nbu), st)))
    print(json.dumps({"leg": "barcode_counts_every_record_its_own_barcode", "n": n, "distinct_barcodes": nb.value, **own}), flush=True)

    for name in a.matrix.split(","):
        ctx.generate(0x1B00005, 0, n, bc_len, umi_len, orig)
        if name != "own_pair":                               # replace the columns (own_pair: random 16-base barcodes, index = i)
            cols = [ctx.alloc(8 * n) for _ in range(3)]
            ctx.deserialize(orig, n, cols[0], cols[1], cols[2])
            ctx.synchronize()
            bc, um, ix = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)
            if name == "1e5x100":                            # 1e5 barcodes x 100 indices, a mean of 4 reads per molecule
                n_umis = max(1, n // (4 * 100_000 * 100))
                for lo in range(0, n, 1 << 26):
                    hi = min(n, lo + (1 << 26))
                    bc[lo:hi] = torch.randint(0, 100_000, (hi - lo,), generator=g, device="cuda", dtype=torch.int64)
                    ix[lo:hi] = torch.randint(0, 100, (hi - lo,), generator=g, device="cuda", dtype=torch.int64)
                    um[lo:hi] = torch.randint(0, n_umis, (hi - lo,), generator=g, device="cuda", dtype=torch.int64)
            elif name == "one_pair":
                bc.fill_(7)
                ix.fill_(3)
            else:
                raise SystemExit(f"unknown --matrix input {name}")
            torch.cuda.synchronize()
            ctx.serialize(cols[0], cols[1], cols[2], n, orig)
            ctx.synchronize()
            for c in cols:
                c.free()
        restore()
        res = {"leg": "count_matrix", "input": name, "n": n}
        res["device_copy"] = rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(t), _dptr(d), 24 * n, st)))
        res["swap_out_of_place"] = rounds(lambda: _check(lib.ibu_records_swap_umi_index(ctx._c, _dptr(d), _dptr(t), n, st)))
        res["swap_in_place"] = rounds(lambda: _check(lib.ibu_records_swap_umi_index(ctx._c, _dptr(d), _dptr(d), n, st)), before=restore)
        res["device_copy_again"] = rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(t), _dptr(d), 24 * n, st)))
        # the four steps, each from the state the one before it leaves
        res["step_swap"] = rounds(lambda: _check(lib.ibu_records_swap_umi_index(ctx._c, _dptr(d), _dptr(d), n, st)), before=restore)
        res["step_sort_swapped"] = rounds(lambda: _check(lib.ibu_sort_records(ctx._c, _dptr(d), _dptr(t), n, st)),
                                          before=lambda: (restore(), _check(lib.ibu_records_swap_umi_index(ctx._c, _dptr(d), _dptr(d), n, st))))
        res["pair_counts_size_query"] = rounds(lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, None, None, None, None, 0, C.byref(npairs), C.byref(ntriples), st)))
        res["step_pair_counts"] = rounds(lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, *[_dptr(o) for o in outs], n, C.byref(npairs), C.byref(ntriples), st)))
        res["reduce"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
        res["barcode_counts_on_the_swapped_sorted_records"] = rounds(
            lambda: _check(lib.ibu_barcode_counts(ctx._c, _dptr(d), n, _dptr(outs[0]), _dptr(outs[1]), _dptr(outs[2]), n, C.byref(nb), C.byref(nbu), st)))
        res["step_swap_back"] = rounds(lambda: _check(lib.ibu_records_swap_umi_index(ctx._c, _dptr(d), _dptr(d), n, st)))
        res["sort_unswapped"] = rounds(lambda: _check(lib.ibu_sort_records(ctx._c, _dptr(d), _dptr(t), n, st)), before=restore)
        ne, nm = C.c_size_t(), C.c_size_t()
        res["count_matrix_call"] = rounds(lambda: _check(lib.ibu_count_matrix(ctx._c, _dptr(d), _dptr(t), n, 0, *[_dptr(o) for o in outs], n, C.byref(ne), C.byref(nm), st)),
                                          before=restore)
        ctx.synchronize()
        assert (ne.value, nm.value) == (npairs.value, ntriples.value), (ne.value, nm.value, npairs.value, ntriples.value)
        assert int(outs[2].download(np.uint64, ne.value).sum()) == n and int(outs[3].download(np.uint64, ne.value).sum()) == nm.value
        res.update({"entries": ne.value, "molecules": nm.value, "csr_rows": nb.value})
        cm = res["count_matrix_call"]["median_ms"]
        res["swap_share_of_call"] = round((res["step_swap"]["median_ms"] + res["step_swap_back"]["median_ms"]) / cm, 3)
        res["swap_vs_copy"] = {"out_of_place": round(res["swap_out_of_place"]["median_ms"] / res["device_copy"]["median_ms"], 3),
                               "in_place": round(res["swap_in_place"]["median_ms"] / res["device_copy"]["median_ms"], 3)}
        res["swap_GBps"] = round(48 * n / res["swap_out_of_place"]["median_ms"] / 1e6)
        print(json.dumps(res), flush=True)


def molecule_fill(torch, i, rpm, cut):
    """Rows i (a tensor of row numbers) of the input of --molecules and --saturation -> their (barcode, umi, index) words: rpm
    consecutive records per molecule, 4096 molecules per barcode, and in a share cut / 2^20 of the molecules the last read (half of
    them: the last two) under the next index."""
    mol, k = i // rpm, i % rpm
    h = ((mol * 0x1E3779B97F4A7C15) >> 20) & 0xFFFFF        # 20 pseudo-random bits per molecule
    second = (h < cut) & (k >= rpm - 1 - (h & 1))
    return mol >> 12, mol & 4095, ((h >> 8) % 100) * 2 + second.to(torch.int64)


def molecule_layout(n, rpm):
    """What molecule_fill lays in rows 0 .. n - 1 -> (barcodes, molecules): the last molecule and the last barcode may be partial."""
    mols = (n + rpm - 1) // rpm
    return (mols + 4095) // 4096, mols


def molecule_legs(a):
    """--molecules: ibu_classify_molecules on resident sorted 16/12 records, timed with events on a side stream (the first round
    is the warm-up), against ibu_pair_counts with outputs, ibu_reduce (one plain read) and ibu_device_copy on the same arrays.
    The records: --reads-per-molecule consecutive records per (barcode, umi), 4096 molecules per barcode; a share
    --second-candidate of the molecules has its last read (half of them: its last two reads — a tie at four reads) under the next
    index."""
    import numpy as np
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib, _lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rpm = a.reads_per_molecule
    cols = [ctx.alloc(8 * n) for _ in range(3)]
    bc, um, ix = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)
    cut = int(a.second_candidate * (1 << 20))
    for lo in range(0, n, 1 << 26):
        hi = min(n, lo + (1 << 26))
        i = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        bc[lo:hi], um[lo:hi], ix[lo:hi] = molecule_fill(torch, i, rpm, cut)
    del i
    torch.cuda.synchronize()
    d, t, d_class = ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(n)
    ctx.serialize(cols[0], cols[1], cols[2], n, d)
    ctx.synchronize()
    for c in cols:
        c.free()
    assert ctx.is_sorted(d, n)
    cap = n // rpm + 16
    outs = [ctx.alloc(8 * cap) for _ in range(4)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    counts = _lib.CMoleculeCounts()
    npairs, ntriples = C.c_size_t(), C.c_size_t()
    res = {"leg": "classify_molecules", "n": n, "reads_per_molecule": rpm, "second_candidate": a.second_candidate}
    res["device_copy"] = rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(t), _dptr(d), 24 * n, st)))
    res["reduce"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
    res["pair_counts"] = rounds(lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, *[_dptr(o) for o in outs], cap, C.byref(npairs), C.byref(ntriples), st)))
    res["classify_classes_only"] = rounds(lambda: _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 0, _dptr(d_class), None, st)))
    res["classify_totals_only"] = rounds(lambda: _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 0, None, C.byref(counts), st)))
    res["classify"] = rounds(lambda: _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 0, _dptr(d_class), C.byref(counts), st)))
    res["classify_tie_first"] = rounds(lambda: _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 1, _dptr(d_class), C.byref(counts), st)))
    res["pair_counts_again"] = rounds(lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, *[_dptr(o) for o in outs], cap, C.byref(npairs), C.byref(ntriples), st)))
    _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 0, _dptr(d_class), C.byref(counts), st))
    ctx.synchronize()
    assert (counts.molecules, counts.candidates) == (npairs.value, ntriples.value)
    assert counts.reads_kept + counts.reads_minor + counts.reads_tied == n
    cls = torch.as_tensor(d_class, device="cuda").view(torch.uint8)[:n]
    assert [int((cls == c).sum()) for c in (0, 1, 2)] == [counts.reads_kept, counts.reads_minor, counts.reads_tied]
    res.update({k: int(getattr(counts, k)) for k in ("molecules", "candidates", "resolved", "tied", "reads_kept", "reads_minor", "reads_tied")})
    pc = min(res["pair_counts"]["median_ms"], res["pair_counts_again"]["median_ms"])
    res["classify_vs_pair_counts"] = round(res["classify"]["median_ms"] / pc, 3)
    res["classes_only_vs_pair_counts"] = round(res["classify_classes_only"]["median_ms"] / pc, 3)
    res["totals_only_vs_pair_counts"] = round(res["classify_totals_only"]["median_ms"] / pc, 3)
    print(json.dumps(res), flush=True)


def knee_layout(torch, n, rpm, device, seed=0x1B0000B):
    """The input of --cells: one cell per 1e4 records of about 2000 molecules (at four reads each), fifty times as many background
    barcodes of 1-3 molecules, shuffled, rpm records per molecule.  -> (umis, starts, ends, n_cells, n_background) per barcode in
    row order: its molecules and its rows [starts, ends).  The rows add up to n EXACTLY: what the rounded random sizes leave over is
    spread over the cells in whole molecules, and the n % rpm records that remain are one more, partial, molecule of the last
    barcode (counted in its umis)."""
    n_cells = max(1, n // 10_000)
    n_bg = 50 * n_cells
    g = torch.Generator(device=device).manual_seed(seed)
    mols = n // rpm
    mean = max(4.0, (mols - 2.0 * n_bg) / n_cells)
    cell = (mean * (0.75 + 0.5 * torch.rand(n_cells, generator=g, device=device, dtype=torch.float64))).to(torch.int64).clamp_(min=4)
    bg = torch.randint(1, 4, (n_bg,), generator=g, device=device, dtype=torch.int64)
    diff = mols - int(cell.sum()) - int(bg.sum())
    cell += diff // n_cells                                  # (floor division and a non-negative remainder, whatever the sign)
    cell[:diff % n_cells] += 1
    if int(cell.min()) < 4:
        raise SystemExit(f"--cells: {n} records are too few for {n_cells} cells and {n_bg} background barcodes")
    umis = torch.cat([cell, bg])[torch.randperm(n_cells + n_bg, generator=g, device=device)]
    reads = umis * rpm
    if n % rpm:
        reads[-1] += n % rpm
        umis[-1] += 1
    ends = torch.cumsum(reads, 0)
    assert int(ends[-1]) == n
    return umis, ends - reads, ends, n_cells, n_bg


def knee_fill(torch, i, starts, ends, rpm):
    """Rows i (a tensor of row numbers) of the layout above -> their (barcode, umi) words."""
    b = torch.bucketize(i, ends, right=True)
    return b, (i - starts[b]) // rpm


def cell_legs(a):
    """--cells: ibu_call_cells in its three modes on resident sorted 16/12 records with a knee, timed with events on a side stream
    (the first round is the warm-up), against ibu_barcode_counts with outputs, ibu_classify_molecules, ibu_reduce (one plain read)
    and ibu_device_copy on the same arrays.  The records: one cell per 1e4 records (1e5 at 1e9) of about 2000 molecules, fifty
    times as many background barcodes of 1-3 molecules scattered among them, --reads-per-molecule records per molecule."""
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib, _lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rpm = a.reads_per_molecule
    umis, starts, ends, n_cells, n_bg = knee_layout(torch, n, rpm, "cuda")
    cols = [ctx.alloc(8 * n) for _ in range(3)]
    bc, um, ix = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)
    for lo in range(0, n, 1 << 26):
        hi = min(n, lo + (1 << 26))
        i = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        bc[lo:hi], um[lo:hi] = knee_fill(torch, i, starts, ends, rpm)
        ix[lo:hi] = 0
    del i
    torch.cuda.synchronize()
    d, t, d_class = ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(n)
    ctx.serialize(cols[0], cols[1], cols[2], n, d)
    ctx.synchronize()
    for c in cols:
        c.free()
    assert ctx.is_sorted(d, n)
    cap = n_cells + n_bg
    outs = [ctx.alloc(8 * cap) for _ in range(3)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    counts, mcounts = _lib.CCellCounts(), _lib.CMoleculeCounts()
    nb, npairs = C.c_size_t(), C.c_size_t()
    cells = lambda mode, param, cls=True, tot=True, flags=0: rounds(lambda: _check(lib.ibu_call_cells(
        ctx._c, _dptr(d), n, mode, param, flags, _dptr(d_class) if cls else None, C.byref(counts) if tot else None, st)))
    res = {"leg": "call_cells", "n": n, "reads_per_molecule": rpm, "cells_laid": n_cells, "background_laid": n_bg}
    res["device_copy"] = rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(t), _dptr(d), 24 * n, st)))
    res["reduce"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
    res["barcode_counts"] = rounds(lambda: _check(lib.ibu_barcode_counts(ctx._c, _dptr(d), n, *[_dptr(o) for o in outs], cap, C.byref(nb), C.byref(npairs), st)))
    res["classify_molecules"] = rounds(lambda: _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 0, _dptr(d_class), C.byref(mcounts), st)))
    res["cells_min"] = cells(ia.CELLS_MIN, 200)
    res["cells_min_classes_only"] = cells(ia.CELLS_MIN, 200, tot=False)
    res["cells_min_totals_only"] = cells(ia.CELLS_MIN, 200, cls=False)
    res["cells_top"] = cells(ia.CELLS_TOP, n_cells)
    res["cells_ordmag"] = cells(ia.CELLS_ORDMAG, n_cells)
    res["cells_ordmag_by_reads"] = cells(ia.CELLS_ORDMAG, n_cells, flags=ia.CELLS_BY_READS)
    res["classify_molecules_again"] = rounds(lambda: _check(lib.ibu_classify_molecules(ctx._c, _dptr(d), n, 0, _dptr(d_class), C.byref(mcounts), st)))
    _check(lib.ibu_call_cells(ctx._c, _dptr(d), n, ia.CELLS_ORDMAG, n_cells, 0, _dptr(d_class), C.byref(counts), st))
    ctx.synchronize()
    res.update({k: int(getattr(counts, k)) for k, _ in _lib.CCellCounts._fields_})
    cm = min(res["classify_molecules"]["median_ms"], res["classify_molecules_again"]["median_ms"])
    for k in ("cells_min", "cells_top", "cells_ordmag"):
        res[k + "_vs_classify_molecules"] = round(res[k]["median_ms"] / cm, 3)
    res["top_minus_min_ms"] = round(res["cells_top"]["median_ms"] - res["cells_min"]["median_ms"], 3)
    res["ordmag_minus_min_ms"] = round(res["cells_ordmag"]["median_ms"] - res["cells_min"]["median_ms"], 3)
    print(json.dumps(res), flush=True)                       # (before the checks: a run that fails one still leaves its times)
    assert counts.barcodes == nb.value and counts.umis_cells + counts.umis_background == npairs.value
    assert counts.reads_cells + counts.reads_background == n
    cls = torch.as_tensor(d_class, device="cuda").view(torch.uint8)[:n]
    assert [int((cls == c).sum()) for c in (0, 1)] == [counts.reads_cells, counts.reads_background]
    assert counts.barcodes == n_cells + n_bg and npairs.value == int(umis.sum()), "every barcode and molecule that was laid"
    assert counts.cells == int((umis >= counts.threshold).sum()), "the cells are the barcodes that were laid with that many molecules"


def metrics_legs(a):
    """--metrics: ibu_barcode_metrics (all columns, with a 60 000-bit feature set and without a set; the size query) and
    ibu_filter_barcodes (with classes, and totals only) on resident {barcode, index, umi} records in sorted order — the knee of
    --cells with every molecule given a feature: four molecules per feature, feature numbers spread over 0 .. 60 000 — timed with
    events on a side stream (the first round is the warm-up).  In the same run and on the same array: ibu_call_cells with classes
    (the same two reads of the records and the same fill: the yardstick), the ibu_pair_counts size query (the same walk, once) and
    ibu_reduce (the plain read: the floor)."""
    import numpy as np
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib, _lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rpm = a.reads_per_molecule
    set_bits = 60_000
    umis, starts, ends, n_cells, n_bg = knee_layout(torch, n, rpm, "cuda")
    cols = [ctx.alloc(8 * n) for _ in range(3)]
    bc, feat, um = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)
    for lo in range(0, n, 1 << 26):
        hi = min(n, lo + (1 << 26))
        i = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        b, m = knee_fill(torch, i, starts, ends, rpm)
        bc[lo:hi], um[lo:hi] = b, m
        feat[lo:hi] = ((m // 4) * 100 + b % 100).clamp_(max=set_bits + 99)   # ascending inside a barcode; a few above the set
    del i, b, m
    torch.cuda.synchronize()
    d, d_class = ctx.alloc(24 * n), ctx.alloc(n)
    ctx.serialize(cols[0], cols[1], cols[2], n, d)           # w1 = the feature, w2 = the umi: what the swap and the sort leave
    ctx.synchronize()
    for c in cols:
        c.free()
    assert ctx.is_sorted(d, n)
    cap = n_cells + n_bg
    outs = [ctx.alloc(8 * cap) for _ in range(6)]
    d_set, _ = ctx.feature_bitmap(np.arange(0, set_bits, 16), set_bits)   # one feature in sixteen

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    nb, npairs, ntriples = C.c_size_t(), C.c_size_t(), C.c_size_t()
    ccounts, fcounts = _lib.CCellCounts(), _lib.CBarcodeFilterCounts()
    lim = _lib.CBarcodeLimits(0, 0, 200, 20 * 500, 0, 0, 1, 10, 1, 0)   # 200 features or more, not absurdly many, at most a tenth of the UMIs in the set
    metrics = lambda s, bits, o, c: rounds(lambda: _check(lib.ibu_barcode_metrics(ctx._c, _dptr(d), n, _dptr(s), bits, 1, *[_dptr(x) for x in o], c, C.byref(nb), st)))
    filt = lambda cls: rounds(lambda: _check(lib.ibu_filter_barcodes(ctx._c, _dptr(d), n, _dptr(d_set), set_bits, 1, C.byref(lim),
                                                                     _dptr(d_class) if cls else None, C.byref(fcounts), st)))
    cells = lambda: rounds(lambda: _check(lib.ibu_call_cells(ctx._c, _dptr(d), n, ia.CELLS_MIN, 200, 0, _dptr(d_class), C.byref(ccounts), st)))
    res = {"leg": "barcode_metrics", "n": n, "reads_per_molecule": rpm, "cells_laid": n_cells, "background_laid": n_bg, "set_bits": set_bits}
    res["reduce"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
    res["pair_counts_size_query"] = rounds(lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, None, None, None, None, 0, C.byref(npairs), C.byref(ntriples), st)))
    res["call_cells_with_classes"] = cells()
    res["metrics_size_query"] = metrics(d_set, set_bits, [None] * 6, 0)
    res["metrics_with_set"] = metrics(d_set, set_bits, outs, cap)
    res["metrics_without_set"] = metrics(None, 0, outs, cap)
    res["filter_with_classes"] = filt(True)
    res["filter_totals_only"] = filt(False)
    res["call_cells_with_classes_again"] = cells()
    res["metrics_with_set_again"] = metrics(d_set, set_bits, outs, cap)
    _check(lib.ibu_filter_barcodes(ctx._c, _dptr(d), n, _dptr(d_set), set_bits, 1, C.byref(lim), _dptr(d_class), C.byref(fcounts), st))   # (the classes the checks look at)
    ctx.synchronize()
    cc = min(res["call_cells_with_classes"]["median_ms"], res["call_cells_with_classes_again"]["median_ms"])
    ws = min(res["metrics_with_set"]["median_ms"], res["metrics_with_set_again"]["median_ms"])
    res["metrics_with_set_vs_call_cells"] = round(ws / cc, 3)
    res["metrics_without_set_vs_call_cells"] = round(res["metrics_without_set"]["median_ms"] / cc, 3)
    res["filter_with_classes_vs_call_cells"] = round(res["filter_with_classes"]["median_ms"] / cc, 3)
    res["with_set_vs_without_set"] = round(ws / res["metrics_without_set"]["median_ms"], 3)
    res["size_query_vs_pair_counts_size_query"] = round(res["metrics_size_query"]["median_ms"] / res["pair_counts_size_query"]["median_ms"], 3)
    res.update({"barcodes": int(fcounts.barcodes), "barcodes_by_class": list(fcounts.barcodes_by_class), "reads_by_class": list(fcounts.reads_by_class)})
    print(json.dumps(res), flush=True)                       # (before the checks: a run that fails one still leaves its times)
    table = [o.download(np.uint64, nb.value) for o in outs]
    assert nb.value == n_cells + n_bg == fcounts.barcodes and int(table[1].sum()) == n and sum(fcounts.reads_by_class) == n
    assert int(table[2].sum()) == npairs.value and int(table[3].sum()) == ntriples.value == int(umis.sum()), "every molecule that was laid"
    assert bool((table[5] <= table[3]).all()) and 0 < int(table[5].sum()) < ntriples.value
    cls = torch.as_tensor(d_class, device="cuda").view(torch.uint8)[:n]
    assert [int((cls == c).sum()) for c in range(4)] == list(fcounts.reads_by_class)


def feature_legs(a):
    """--features: ibu_feature_metrics (all three columns; reads only) and ibu_filter_features (the class pass alone; with its
    totals; metrics and filter together) on the resident {barcode, index, umi} array of --metrics — the knee of --cells with four
    molecules per feature, feature numbers spread over 0 .. 60 000 — with n_features = 60 000, so that a few records are out of
    range; timed with events on a side stream (the first round is the warm-up).  In the same run and on the same array: the
    ibu_pair_counts size query (the same walk, once), ibu_reduce (the plain read) and ibu_call_cells with classes.  Then a second
    leg on the same array with a tenth of all pairs given to ONE feature (pairs picked by a hash, so the array is no longer sorted
    inside a barcode, which the metrics do not need): the hot counter every real sample has."""
    import numpy as np
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib, _lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rpm = a.reads_per_molecule
    nf, hot = 60_000, 7
    umis, starts, ends, n_cells, n_bg = knee_layout(torch, n, rpm, "cuda")
    cols = [ctx.alloc(8 * n) for _ in range(3)]
    bc, feat, um = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)

    def fill(hot_share):
        for lo in range(0, n, 1 << 26):
            hi = min(n, lo + (1 << 26))
            i = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
            b, m = knee_fill(torch, i, starts, ends, rpm)
            bc[lo:hi], um[lo:hi] = b, m
            f = ((m // 4) * 100 + b % 100).clamp_(max=nf + 99)   # ascending inside a barcode; a few at and above n_features
            if hot_share:
                h = (((b * 0x9E3779B1 + m // 4) * 0x1E3779B97F4A7C15) >> 20) & 0xFFFFF   # 20 pseudo-random bits per pair
                f = torch.where(h % hot_share == 0, torch.full_like(f, hot), f)
            feat[lo:hi] = f
        torch.cuda.synchronize()
        ctx.serialize(cols[0], cols[1], cols[2], n, d)       # w1 = the feature, w2 = the umi: what the swap and the sort leave
        ctx.synchronize()

    d, d_class = ctx.alloc(24 * n), ctx.alloc(n)
    table = [ctx.alloc(8 * nf) for _ in range(3)]
    fill(0)
    assert ctx.is_sorted(d, n)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    npairs, ntriples = C.c_size_t(), C.c_size_t()
    totals = (C.c_uint64 * 4)()
    ccounts, fcounts = _lib.CCellCounts(), _lib.CFeatureFilterCounts()
    lim = _lib.CFeatureLimits(0, 0, 0, 0, 3, 0)                  # min_cells = 3
    metrics = lambda given, t: _check(lib.ibu_feature_metrics(ctx._c, _dptr(d), n, 1, nf, 0, *[_dptr(x) for x in given], t, st))
    filt = lambda cls, cnt: _check(lib.ibu_filter_features(ctx._c, _dptr(d), n, 1, nf, *[_dptr(x) for x in table], C.byref(lim),
                                                           _dptr(d_class) if cls else None, None, C.byref(fcounts) if cnt else None, st))
    pairs = lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, None, None, None, None, 0, C.byref(npairs), C.byref(ntriples), st))

    def leg():
        r = {}
        r["reduce"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
        r["pair_counts_size_query"] = rounds(pairs)
        r["call_cells_with_classes"] = rounds(lambda: _check(lib.ibu_call_cells(ctx._c, _dptr(d), n, ia.CELLS_MIN, 200, 0, _dptr(d_class), C.byref(ccounts), st)))
        r["metrics_three_columns"] = rounds(lambda: metrics(table, totals))
        r["metrics_reads_only"] = rounds(lambda: metrics([table[0], None, None], totals))
        r["metrics_three_columns_no_totals"] = rounds(lambda: metrics(table, None))
        r["pair_counts_size_query_again"] = rounds(pairs)
        r["metrics_three_columns_again"] = rounds(lambda: metrics(table, totals))
        r["filter_class_pass"] = rounds(lambda: filt(True, False))
        r["filter_with_classes_and_totals"] = rounds(lambda: filt(True, True))
        r["filter_totals_only"] = rounds(lambda: filt(False, True))
        r["metrics_and_filter"] = rounds(lambda: (metrics(table, None), filt(True, True)))
        pq = min(r["pair_counts_size_query"]["median_ms"], r["pair_counts_size_query_again"]["median_ms"])
        m3 = min(r["metrics_three_columns"]["median_ms"], r["metrics_three_columns_again"]["median_ms"])
        for k in ("metrics_reads_only", "filter_class_pass", "filter_with_classes_and_totals", "metrics_and_filter"):
            r[k + "_vs_size_query"] = round(r[k]["median_ms"] / pq, 3)
            r[k + "_vs_reduce"] = round(r[k]["median_ms"] / r["reduce"]["median_ms"], 3)
            r[k + "_vs_call_cells"] = round(r[k]["median_ms"] / r["call_cells_with_classes"]["median_ms"], 3)
        r["metrics_three_columns_vs_size_query"] = round(m3 / pq, 3)
        r["metrics_three_columns_vs_reduce"] = round(m3 / r["reduce"]["median_ms"], 3)
        r["metrics_three_columns_vs_call_cells"] = round(m3 / r["call_cells_with_classes"]["median_ms"], 3)
        r.update({"pairs": npairs.value, "triples": ntriples.value, "totals": list(totals), "features_by_class": list(fcounts.features_by_class),
                  "reads_by_class": list(fcounts.reads_by_class)})
        return r, m3

    def checks():
        got = [t.download(np.uint64, nf) for t in table]
        assert totals[0] + totals[3] == n == sum(fcounts.reads_by_class) and int(got[0].sum()) == totals[0]
        assert int(got[1].sum()) == totals[1] <= ntriples.value and int(got[2].sum()) == totals[2] <= npairs.value
        assert sum(fcounts.features_by_class) == nf and fcounts.features_by_class[1] == int((got[2] < 3).sum())
        cls = torch.as_tensor(d_class, device="cuda").view(torch.uint8)[:n]
        assert [int((cls == c).sum()) for c in range(4)] == list(fcounts.reads_by_class) and fcounts.reads_by_class[3] == totals[3]
        return got

    res = {"leg": "feature_metrics", "n": n, "reads_per_molecule": rpm, "cells_laid": n_cells, "background_laid": n_bg, "n_features": nf}
    res["uniform"], m3_uniform = leg()
    print(json.dumps(res), flush=True)                       # (before the checks: a run that fails one still leaves its times)
    got = checks()
    assert int(umis.sum()) == ntriples.value, "every molecule that was laid"
    fill(10)
    res["hot"], m3_hot = leg()
    res["hot_vs_uniform_three_columns"] = round(m3_hot / m3_uniform, 3)
    res["hot_vs_uniform_reads_only"] = round(res["hot"]["metrics_reads_only"]["median_ms"] / res["uniform"]["metrics_reads_only"]["median_ms"], 3)
    got = checks()
    res["hot_feature_share_of_pairs"] = round(int(got[2][hot]) / max(1, npairs.value), 4)
    print(json.dumps(res), flush=True)


def saturation_legs(a):
    """--saturation: the ten-point ibu_saturation_curve, and ibu_subsample_class + ibu_select_records at fraction 0.5, on resident
    sorted 16/12 records (the array --molecules lays), timed with events on a side stream (the first round is the warm-up).  In the
    same run and on the same array: ibu_reduce (the plain read: the floor), the ibu_pair_counts size query (the same walk over the
    same bytes: the curve's yardstick), ibu_select_records alone on the same classes, and a fill of n bytes (the subsample kernel's
    yardstick).  Before anything is timed, the 1.0 point of the curve is checked against ibu_pair_counts / ibu_barcode_counts and
    against what was laid."""
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib, _lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rpm = a.reads_per_molecule
    cols = [ctx.alloc(8 * n) for _ in range(3)]
    bc, um, ix = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)
    cut = int(a.second_candidate * (1 << 20))
    for lo in range(0, n, 1 << 26):
        hi = min(n, lo + (1 << 26))
        i = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        bc[lo:hi], um[lo:hi], ix[lo:hi] = molecule_fill(torch, i, rpm, cut)
    del i
    torch.cuda.synchronize()
    d, t, d_class = ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(n)
    ctx.serialize(cols[0], cols[1], cols[2], n, d)
    ctx.synchronize()
    for c in cols:
        c.free()
    assert ctx.is_sorted(d, n)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    K = 10
    seed = 0x1B0000C
    ts = (C.c_uint64 * K)(*[ia.sample_threshold(j / K) if j < K else (1 << 64) - 1 for j in range(1, K + 1)])
    pts = (_lib.CSaturationPoint * K)()
    npairs, ntriples, nb, nbu, kept, sel = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    curve = lambda: _check(lib.ibu_saturation_curve(ctx._c, _dptr(d), n, 0, seed, ts, K, pts, st))
    pairs = lambda: _check(lib.ibu_pair_counts(ctx._c, _dptr(d), n, None, None, None, None, 0, C.byref(npairs), C.byref(ntriples), st))
    # the check, before anything is timed
    curve()
    pairs()
    _check(lib.ibu_barcode_counts(ctx._c, _dptr(d), n, None, None, None, 0, C.byref(nb), C.byref(nbu), st))
    last = pts[K - 1]
    assert (last.reads, last.barcodes, last.molecules) == (n, nb.value, npairs.value), ((last.reads, last.barcodes, last.molecules), n, nb.value, npairs.value)
    assert (nb.value, npairs.value) == molecule_layout(n, rpm), "every barcode and molecule that was laid"
    assert all(pts[j].reads <= pts[j + 1].reads and pts[j].molecules <= pts[j + 1].molecules for j in range(K - 1))
    half = ia.sample_threshold(0.5)
    sub = lambda want=True: _check(lib.ibu_subsample_class(ctx._c, n, 0, seed, half, _dptr(d_class), C.byref(kept) if want else None, st))
    select = lambda: _check(lib.ibu_select_records(ctx._c, _dptr(d), _dptr(d_class), n, 1 << ia.SAMPLE_KEPT, _dptr(t), n, C.byref(sel), st))
    sub()
    select()
    ctx.synchronize()
    assert kept.value == sel.value == pts[4].reads, (kept.value, sel.value, pts[4].reads)
    cls = torch.as_tensor(d_class, device="cuda").view(torch.uint8)[:n]
    res = {"leg": "saturation", "n": n, "reads_per_molecule": rpm, "points": K,
           "curve": [{"fraction": (j + 1) / K, "reads": pts[j].reads, "barcodes": pts[j].barcodes, "molecules": pts[j].molecules,
                      "saturation": round(1 - pts[j].molecules / max(1, pts[j].reads), 6)} for j in range(K)]}
    res["reduce"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
    res["pair_counts_size_query"] = rounds(pairs)
    res["saturation_curve"] = rounds(curve)
    res["pair_counts_size_query_again"] = rounds(pairs)
    with torch.cuda.stream(side):
        res["fill_n_bytes"] = rounds(lambda: cls.fill_(1))
    res["subsample_class"] = rounds(lambda: sub(False))
    res["subsample_class_with_count"] = rounds(sub)
    res["select_records"] = rounds(select)
    res["subsample_and_select"] = rounds(lambda: (sub(False), select()))
    res["reduce_again"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(d), n, st)))
    pq = min(res["pair_counts_size_query"]["median_ms"], res["pair_counts_size_query_again"]["median_ms"])
    rd = min(res["reduce"]["median_ms"], res["reduce_again"]["median_ms"])
    res["curve_vs_size_query"] = round(res["saturation_curve"]["median_ms"] / pq, 3)
    res["curve_vs_reduce"] = round(res["saturation_curve"]["median_ms"] / rd, 3)
    res["subsample_vs_fill"] = round(res["subsample_class"]["median_ms"] / res["fill_n_bytes"]["median_ms"], 3)
    res["subsample_and_select_vs_select"] = round(res["subsample_and_select"]["median_ms"] / res["select_records"]["median_ms"], 3)
    print(json.dumps(res), flush=True)


MTX_ROW, MTX_BC_LEN = 1999, 16                                  # --mtx: entries per barcode (no multiple of a unit of 2048), bases per barcode


def mtx_fill(torch, i):
    """--mtx: entry i of the synthetic entry table -> (barcode, index, umis, reads) as int64 tensors, a pure function of i (replayed
    on the CPU by tests/test_mtx_tools.py).  Rows of MTX_ROW entries; the barcode of row r is r scattered over 32 bits by an odd
    multiplier, so neighbouring rows differ; the index ascends inside a row in steps of 17 (up to five digits); the UMI count is
    1 .. 20 with one entry in 1024 in the thousands, the reads three times that and one."""
    row = i // MTX_ROW
    bc = (row * 0x9E3779B1) & 0xFFFFFFFF
    idx = (i % MTX_ROW) * 17
    h = ((i * 0x9E3779B1) >> 7) & 0xFFFFF
    umis = 1 + h % 20 + torch.where(h % 1024 == 0, h // 64, torch.zeros_like(h))
    return bc, idx, umis, 3 * umis + 1


def mtx_layout(n):
    """-> (rows, n_features) of the table mtx_fill lays for n entries."""
    return (n + MTX_ROW - 1) // MTX_ROW, (MTX_ROW - 1) * 17 + 1


def mtx_traffic(n, text_bytes):
    """The bytes ibu_matrix_market_body moves for n entries and text_bytes of text: the three columns read twice and the text written
    once — and the size of the ibu_device_copy (read + write of every byte) that moves as many."""
    total = 2 * 3 * 8 * n + text_bytes
    return total, total // 2


def mtx_table(torch, ia, ctx, n):
    """The resident entry table of --mtx and --rowtop, laid by mtx_fill -> (three, d_idx, d_ord, d_umis, d_bc, d_reads, views): `three` holds
    index | row ordinal | umis back to back (ibu_reduce reads them as n records), views are int64 tensors over bc, idx, umis, reads."""
    three = ctx.alloc(24 * n)
    d_idx, d_ord, d_umis = (ia.DeviceBuffer.wrap(ctx, three.ptr + 8 * n * k, 8 * n) for k in range(3))
    d_bc, d_reads = ctx.alloc(8 * n), ctx.alloc(8 * n)
    views = [torch.as_tensor(b, device="cuda").view(torch.int64) for b in (d_bc, d_idx, d_umis, d_reads)]
    for lo in range(0, n, 1 << 26):
        hi = min(n, lo + (1 << 26))
        for v, x in zip(views, mtx_fill(torch, torch.arange(lo, hi, device="cuda", dtype=torch.int64))):
            v[lo:hi] = x
    torch.cuda.synchronize()
    return three, d_idx, d_ord, d_umis, d_bc, d_reads, views


ROWTOP_SET_EVERY = 3                                             # --rowtop: the set holds every third feature number


def rowtop_legs(a):
    """--rowtop: the per-row top-2 on the resident entry table of --mtx (mtx_table: the same arrays, one run), timed with events on a
    side stream (the first round is the warm-up): ibu_matrix_row_top with all five outputs, without a set and with one (every third
    feature number: one gathered bitmap word per entry), its size query, and ibu_assign_rows on the columns it left (classes and
    totals) — against ibu_matrix_rows with all three outputs and ibu_reduce over the three columns (one plain read of 24 B per
    entry) on the same arrays.  Before anything is timed the result is checked against what was laid: the rows, and per row the
    largest UMI count, its feature, the runner-up, the sum and the entries, computed with torch from the same columns."""
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib, _lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rows_laid, nf = mtx_layout(n)
    assert n >= MTX_ROW, "--rowtop wants at least one full row"
    three, d_idx, d_ord, d_umis, d_bc, d_reads, views = mtx_table(torch, ia, ctx, n)
    d_keys, d_ptr = ctx.alloc(8 * rows_laid), ctx.alloc(8 * (rows_laid + 1))
    outs = [ctx.alloc(8 * rows_laid) for _ in range(5)]
    d_class = ctx.alloc(rows_laid)
    fset = ctx.feature_bitmap(range(0, nf, ROWTOP_SET_EVERY), nf)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    nr = C.c_size_t()
    rows = lambda o, cap: _check(lib.ibu_matrix_rows(ctx._c, _dptr(d_bc), n, *[_dptr(x) for x in o], cap, C.byref(nr), st))
    top = lambda s, o, cap: _check(lib.ibu_matrix_row_top(ctx._c, _dptr(d_bc), _dptr(d_idx), _dptr(d_umis), n, _dptr(s[0]) if s else None,
                                                         s[1] if s else 0, *[_dptr(x) for x in o], cap, C.byref(nr), st))
    rule, counts = _lib.CAssignRule(2, 1, 2), _lib.CAssignCounts()
    assign = lambda: _check(lib.ibu_assign_rows(ctx._c, _dptr(outs[1]), _dptr(outs[2]), _dptr(outs[3]), rows_laid, C.byref(rule), _dptr(d_class),
                                                C.byref(counts), st))
    # the check, before anything is timed: a row is MTX_ROW consecutive entries (the last one shorter)
    got = [torch.as_tensor(o, device="cuda").view(torch.int64)[:rows_laid] for o in outs]
    pad = rows_laid * MTX_ROW - n
    for s in (None, fset):
        top(s, outs, rows_laid)
        ctx.synchronize()
        assert nr.value == rows_laid, (nr.value, rows_laid)
        part = torch.ones(n, dtype=torch.bool, device="cuda") if s is None else views[1] % ROWTOP_SET_EVERY == 0
        v = torch.nn.functional.pad(torch.where(part, views[2], torch.zeros_like(views[2])), (0, pad)).view(rows_laid, MTX_ROW)
        k = torch.nn.functional.pad(part.to(torch.int64), (0, pad)).view(rows_laid, MTX_ROW)
        best, at = v.max(dim=1)                                  # torch does not promise the FIRST maximum: the key is checked through its value
        assert bool((got[1] == best).all()) and bool((got[3] == v.sum(dim=1)).all()) and bool((got[4] == k.sum(dim=1)).all())
        key_at = got[0] // 17                                    # idx = 17 x the position in the row
        assert bool((v.gather(1, key_at.view(-1, 1)).view(-1) == best).all())
        pos = torch.arange(MTX_ROW, device="cuda", dtype=torch.int64).view(1, -1)
        first_at = torch.where(v == best.view(-1, 1), pos, torch.full_like(pos, MTX_ROW)).min(dim=1).values
        assert bool((key_at == first_at).all())
        others = v.clone()
        others.scatter_(1, first_at.view(-1, 1), 0)
        assert bool((got[2] == others.max(dim=1).values).all())
        del v, k, others
    res = {"leg": "rowtop", "n": n, "rows": rows_laid, "n_features": nf, "set_every": ROWTOP_SET_EVERY}
    res["reduce_three_columns"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(three), n, st)))
    res["matrix_rows_all_outputs"] = rounds(lambda: rows([d_ord, d_keys, d_ptr], rows_laid))
    res["row_top_size_query"] = rounds(lambda: top(None, [None] * 5, 0))
    res["row_top_all_outputs"] = rounds(lambda: top(None, outs, rows_laid))
    res["row_top_all_outputs_with_set"] = rounds(lambda: top(fset, outs, rows_laid))
    res["assign_rows"] = rounds(assign)
    res["reduce_three_columns_again"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(three), n, st)))
    rd = min(res["reduce_three_columns"]["median_ms"], res["reduce_three_columns_again"]["median_ms"])
    assert counts.rows == rows_laid == counts.assigned + counts.none + counts.mixed
    res["assign_counts"] = [int(counts.assigned), int(counts.none), int(counts.mixed)]
    for leg in ("row_top_size_query", "row_top_all_outputs", "row_top_all_outputs_with_set", "matrix_rows_all_outputs"):
        res[leg + "_vs_reduce"] = round(res[leg]["median_ms"] / rd, 3)
    for leg in ("row_top_all_outputs", "row_top_all_outputs_with_set"):
        res[leg + "_vs_matrix_rows"] = round(res[leg]["median_ms"] / res["matrix_rows_all_outputs"]["median_ms"], 3)
    print(json.dumps(res), flush=True)


def mtx_legs(a):
    """--mtx: the matrix export on a resident entry table of --records entries (mtx_fill), one run on one set of arrays, timed with
    events on a side stream (the first round is the warm-up): ibu_matrix_rows (size query; all three outputs), ibu_matrix_market_body
    (the size query = the length pass; the full call = length pass + write pass, the write pass being the difference), against
    ibu_device_copy of as many bytes as the body moves (mtx_traffic) and ibu_reduce over the three columns (one plain read of 24 B
    per entry); then the wall time of the host loop examples/count_file.cpp prints with (tools/mtx_host_loop.cpp, one printf per entry
    to /dev/null) on the same columns, downloaded.  Before anything is timed the row structure is checked against what was laid."""
    import subprocess
    import tempfile
    import numpy as np
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records.split(",")[0]))
    rows_laid, nf = mtx_layout(n)
    assert n >= MTX_ROW, "--mtx wants at least one full row"
    three, d_idx, d_ord, d_umis, d_bc, d_reads, views = mtx_table(torch, ia, ctx, n)
    d_keys, d_ptr = ctx.alloc(8 * rows_laid), ctx.alloc(8 * (rows_laid + 1))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn):
        v = [timed(fn) for _ in range(a.rounds + 1)][1:]
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    nr, nb, mx = C.c_size_t(), C.c_size_t(), (C.c_uint64 * 3)()
    rows = lambda outs, cap: _check(lib.ibu_matrix_rows(ctx._c, _dptr(d_bc), n, *[_dptr(o) for o in outs], cap, C.byref(nr), st))
    body = lambda text, cap: _check(lib.ibu_matrix_market_body(ctx._c, _dptr(d_idx), _dptr(d_ord), _dptr(d_umis), n, 1, 1, _dptr(text), cap,
                                                               C.byref(nb), mx, st))
    # the check, before anything is timed
    rows([d_ord, d_keys, d_ptr], rows_laid)
    ctx.synchronize()
    assert nr.value == rows_laid, (nr.value, rows_laid)
    ptr = torch.as_tensor(d_ptr, device="cuda").view(torch.int64)[:rows_laid + 1]
    assert bool((ptr == torch.clamp(torch.arange(rows_laid + 1, device="cuda", dtype=torch.int64) * MTX_ROW, max=n)).all())
    body(None, 0)
    text_bytes = nb.value
    assert tuple(mx) == (nf, rows_laid, int(views[2].max())), (tuple(mx), nf, rows_laid)
    d_text = ctx.alloc(text_bytes + 1)
    body(ia.DeviceBuffer.wrap(ctx, d_text.ptr + 1, text_bytes), text_bytes)   # an odd address
    ctx.synchronize()
    head = d_text.download(np.uint8, 64, 1).tobytes().split(b"\n")[0]
    assert head == b"1 1 %d" % int(views[2][0]), head
    total, copy_bytes = mtx_traffic(n, text_bytes)
    src, dst = ctx.alloc(copy_bytes), ctx.alloc(copy_bytes)
    res = {"leg": "mtx", "n": n, "rows": rows_laid, "n_features": nf, "text_bytes": text_bytes, "bytes_per_line": round(text_bytes / n, 2),
           "body_traffic_bytes": total, "copy_bytes": copy_bytes}
    res["device_copy"] = rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(dst), _dptr(src), copy_bytes, st)))
    res["reduce_three_columns"] = rounds(lambda: _check(lib.ibu_reduce(ctx._c, _dptr(three), n, st)))
    res["matrix_rows_size_query"] = rounds(lambda: rows([None] * 3, 0))
    res["matrix_rows_all_outputs"] = rounds(lambda: rows([d_ord, d_keys, d_ptr], rows_laid))
    res["body_size_query"] = rounds(lambda: body(None, 0))
    res["body_full_call"] = rounds(lambda: body(d_text, text_bytes))
    res["device_copy_again"] = rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(dst), _dptr(src), copy_bytes, st)))
    cp = min(res["device_copy"]["median_ms"], res["device_copy_again"]["median_ms"])
    res["body_write_pass_ms"] = round(res["body_full_call"]["median_ms"] - res["body_size_query"]["median_ms"], 3)   # a difference, not a timing
    res["body_full_call_vs_copy"] = round(res["body_full_call"]["median_ms"] / cp, 3)
    res["body_size_query_vs_reduce"] = round(res["body_size_query"]["median_ms"] / res["reduce_three_columns"]["median_ms"], 3)
    res["matrix_rows_all_outputs_vs_reduce"] = round(res["matrix_rows_all_outputs"]["median_ms"] / res["reduce_three_columns"]["median_ms"], 3)
    print(json.dumps(res), flush=True)                       # (before the host loop: a run that is cut short there still leaves its times)
    host_n = min(n, int(float(a.host_entries))) if a.host_entries else n
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "mtx_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "mtx_host_loop.cpp"), "-o", so])
        loop = C.CDLL(so).mtx_host_loop
        loop.restype, loop.argtypes = C.c_double, [C.c_void_p] * 4 + [C.c_size_t, C.c_uint32, C.c_char_p]
        t0 = time.perf_counter()
        cols = [b.download(np.uint64, host_n) for b in (d_bc, d_idx, d_umis, d_reads)]
        res["download_four_columns_s"] = round(time.perf_counter() - t0, 3)
        s = loop(*[c.ctypes.data for c in cols], host_n, MTX_BC_LEN, b"/dev/null")
        assert s >= 0
    res["host_loop_entries"] = host_n
    res["host_loop_s"] = round(s, 3)
    res["host_loop_s_per_1e8"] = round(s * 1e8 / host_n, 3)
    t0 = time.perf_counter()
    got = d_text.download(np.uint8, text_bytes)
    res["download_text_s"] = round(time.perf_counter() - t0, 3)
    assert got[-1] == 10 and int((got == 10).sum()) == n
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mtx", action="store_true", help="the ibu_matrix_rows / ibu_matrix_market_body legs instead of the barcode leg")
    ap.add_argument("--host-entries", default="", help="--mtx: the host loop runs over this many entries (default: all)")
    ap.add_argument("--saturation", action="store_true", help="the ibu_saturation_curve / ibu_subsample_class legs instead of the barcode leg")
    ap.add_argument("--metrics", action="store_true", help="the ibu_barcode_metrics / ibu_filter_barcodes legs instead of the barcode leg")
    ap.add_argument("--features", action="store_true", help="the ibu_feature_metrics / ibu_filter_features legs instead of the barcode leg")
    ap.add_argument("--cells", action="store_true", help="the ibu_call_cells legs instead of the barcode leg")
    ap.add_argument("--molecules", action="store_true", help="the ibu_classify_molecules legs instead of the barcode leg")
    ap.add_argument("--reads-per-molecule", type=int, default=4)
    ap.add_argument("--second-candidate", type=float, default=0.05, help="--molecules: the share of molecules with a second index")
    ap.add_argument("--matrix", default="", help="count-matrix legs instead of the barcode leg: a comma list of inputs out of 1e5x100, own_pair, one_pair")
    ap.add_argument("--records", default="1e9")
    ap.add_argument("--lens", default="10,12;16,12")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--whitelist", type=int, default=0, help="K > 0: barcodes drawn from K distinct ones, skewed (rank ~ K u^3), as tools/sortbench.py --whitelist")
    ap.add_argument("--rowtop", action="store_true", help="the ibu_matrix_row_top / ibu_assign_rows legs on the entry table of --mtx instead of the barcode leg")
    a = ap.parse_args()
    if a.rowtop:
        return rowtop_legs(a)
    if a.mtx:
        return mtx_legs(a)
    if a.saturation:
        return saturation_legs(a)
    if a.metrics:
        return metrics_legs(a)
    if a.features:
        return feature_legs(a)
    if a.molecules:
        return molecule_legs(a)
    if a.cells:
        return cell_legs(a)
    if a.matrix:
        return matrix_legs(a)
    if a.whitelist:
        import torch                                         # before the library, as bench.py does
        torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _dptr, _check, lib

    ctx = ia.Context(0)
    for n in (int(float(x)) for x in a.records.split(",")):
        d, t = ctx.alloc(24 * n), ctx.alloc(24 * n)
        for lens in a.lens.split(";"):
            bc_len, umi_len = (int(x) for x in lens.split(","))
            ctx.generate(0x1B00005, 0, n, bc_len, umi_len, d)
            if a.whitelist:                                    # replace the barcode column
                cols = [ctx.alloc(8 * n) for _ in range(3)]
                ctx.deserialize(d, n, cols[0], cols[1], cols[2])
                g = torch.Generator(device="cuda").manual_seed(0x1B00007)
                wl = _rand_bits(torch, g, 2 * bc_len, a.whitelist)
                bc = torch.as_tensor(cols[0], device="cuda").view(torch.int64)
                for lo in range(0, n, 1 << 26):
                    hi = min(n, lo + (1 << 26))
                    u = torch.rand(hi - lo, generator=g, device="cuda", dtype=torch.float64)
                    bc[lo:hi] = wl[(u * u * u * a.whitelist).to(torch.int64).clamp_(max=a.whitelist - 1)]
                del u
                torch.cuda.synchronize()
                ctx.serialize(cols[0], cols[1], cols[2], n, d)
                for c in cols:
                    c.free()
            ctx.sort_records(d, t, n)
            ctx.synchronize()
            nb, npairs = C.c_size_t(), C.c_size_t()
            q = []
            for _ in range(a.rounds + 1):
                t0 = time.perf_counter()
                _check(lib.ibu_barcode_counts(ctx._c, _dptr(d), n, None, None, None, 0, C.byref(nb), C.byref(npairs), None))
                q.append(time.perf_counter() - t0)
            u = nb.value
            d_b, d_c, d_u = ctx.alloc(8 * u), ctx.alloc(8 * u), ctx.alloc(8 * u)
            e = []
            for _ in range(a.rounds + 1):
                t0 = time.perf_counter()
                _check(lib.ibu_barcode_counts(ctx._c, _dptr(d), n, _dptr(d_b), _dptr(d_c), _dptr(d_u), u, C.byref(nb),
                                              C.byref(npairs), None))
                ctx.synchronize()
                e.append(time.perf_counter() - t0)
            import numpy as np
            counts = d_c.download(np.uint64)
            assert int(counts.sum()) == n and int(d_u.download(np.uint64).sum()) == npairs.value
            qs, es = statistics.median(q[1:]), statistics.median(e[1:])
            # algorithmic bytes: the barcode and UMI words of every record once per pass (16 B; the hardware fetches the
            # whole 24-byte record) + 24 B per distinct barcode written; the emit call runs the count pass again
            print(json.dumps({"n": n, "lens": [bc_len, umi_len], "whitelist": a.whitelist or None, "distinct_barcodes": u, "barcode_umi_pairs": npairs.value,
                              "size_query_ms": round(qs * 1e3, 3), "emit_call_ms": round(es * 1e3, 3),
                              "size_query_GBps_of_24B": round(24 * n / qs / 1e9),
                              "emit_call_GBps_of_24B_x2": round((48 * n + 24 * u) / es / 1e9)}), flush=True)
            for x in (d_b, d_c, d_u):
                x.free()
        d.free()
        t.free()


if __name__ == "__main__":
    main()
