#!/usr/bin/env python3
"""Throughput of ibu_sort_records on device-resident records.
  python tools/sortbench.py [--records 1e8,1e9] [--lens 16,12] [--rounds 3]
  python tools/sortbench.py --merge [--records 1e9]   the merge of sorted records beside the copy, the field exchange and the sort"""
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


def shards_main(a, ia, bc_len, umi_len):
    k = a.shards
    ctxs = [ia.Context(0) for _ in range(k)]
    if a.sort_first:                                           # the round-3 form of the call (every shard sorted, exchanged, sorted again)
        ctxs[0].set_option("sort_compact", 0)
    for n in (int(float(x)) for x in a.records.split(",")):
        per, cap = n // k, int(n // k * 1.25) + k + 1
        bufs = [(c.alloc(24 * cap), c.alloc(24 * cap)) for c in ctxs]
        ts, outs = [], None
        for _ in range(a.rounds + 1):
            for i, (c, (d, t)) in enumerate(zip(ctxs, bufs)):     # shard i = rows [i per, (i + 1) per) of the generator's stream
                c.generate(0x1B00005, i * per, per, bc_len, umi_len, d)
                c.synchronize()
            t0 = time.perf_counter()
            outs = ia.Context.sort_records_contexts(ctxs, [(d, t, per, cap) for d, t in bufs])
            ts.append(time.perf_counter() - t0)
        assert sum(outs) == per * k and all(c.is_sorted(d, m) for c, (d, _), m in zip(ctxs, bufs, outs))
        sec = statistics.median(ts[1:])
        print(json.dumps({"n": per * k, "lens": [bc_len, umi_len], "contexts_on_device_0": k, "form": "sort first (forced)" if a.sort_first else "default",
                          "seconds": round(sec, 4),
                          "M_records_per_s": round(per * k / sec / 1e6, 1), "records_per_shard_after": outs,
                          "note": "one GPU: the K local sorts share it and the exchange is a device-local copy"}), flush=True)
        for d, t in bufs:
            d.free()
            t.free()


def merge_main(a):
    """ibu_merge_sorted on two equal sorted halves of n resident records (three shapes) and ibu_merge_sorted_runs at k = 2, 8, 64,
    beside the yardsticks on the same arrays in the same process: ibu_device_copy of n * 24 bytes, ibu_records_swap_umi_index out
    of place and ibu_sort_records of the concatenation.  HIP-event times on one side stream; one warm-up and --rounds repeats each;
    one JSON line."""
    import torch
    torch.cuda.init()
    import ibu_amd as ia
    from ibu_amd import _check, _dptr, lib

    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float((a.records or "1e9").split(",")[0])) // 128 * 128   # whole runs at every k
    bc_len, umi_len = (int(x) for x in a.lens.split(","))
    half = n // 2
    orig, d, t = ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(24 * n)
    src = ctx.alloc(n)
    at = lambda buf, first, count: ia.DeviceBuffer.wrap(ctx, buf.ptr + 24 * first, 24 * max(count, 1))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(fn, before=None):
        v = []
        for _ in range(a.rounds + 1):
            if before:
                before()
            torch.cuda.synchronize()
            ctx.synchronize()
            v.append(timed(fn))
        v = v[1:]                                              # the first is the warm-up
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    def restore():                                             # d = the records as `orig` holds them
        ctx.copy(d, orig, 24 * n)
        ctx.synchronize()

    def sort_runs(k):                                          # orig = k sorted runs of n / k records
        per = n // k
        for j in range(k):
            ctx.sort_records(at(orig, j * per, per), t, per)
        ctx.synchronize()

    def random_records():                                      # 16/12 keys, index = row number (below 2^32)
        ctx.generate(0x1B0000A, 0, n, bc_len, umi_len, orig)
        ctx.synchronize()

    def whitelist_records(k=100_000):                          # barcodes from k distinct ones, skewed (rank ~ k u^3): long runs of equal barcode
        g = torch.Generator(device="cuda").manual_seed(0x1B0000B)
        cols = [ctx.alloc(8 * n) for _ in range(3)]
        wl = _rand_bits(torch, g, 2 * bc_len, k)
        bc, um, ix = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols)
        step = 1 << 26
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            u = torch.rand(hi - lo, generator=g, device="cuda", dtype=torch.float64)
            bc[lo:hi] = wl[(u * u * u * k).to(torch.int64).clamp_(max=k - 1)]
            um[lo:hi] = _rand_bits(torch, g, 2 * umi_len, hi - lo)
            ix[lo:hi] = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        del u, bc, um, ix
        torch.cuda.synchronize()
        ctx.serialize(cols[0], cols[1], cols[2], n, orig)
        ctx.synchronize()
        for c in cols:
            c.free()

    def two_way(shape):
        if shape == "disjoint":                                # one sort of everything: the halves are disjoint key ranges
            sort_runs(1)
        else:
            sort_runs(2)
        a_, b_ = at(orig, 0, half), at(orig, half, n - half)
        merge = lambda s: _check(lib.ibu_merge_sorted(ctx._c, _dptr(a_), half, _dptr(b_), n - half, _dptr(d), _dptr(s), st))
        res = {"merge": rounds(lambda: merge(None)), "merge_with_source": rounds(lambda: merge(src)),
               "copy": rounds(lambda: _check(lib.ibu_device_copy(ctx._c, _dptr(d), _dptr(orig), 24 * n, st))),
               "swap_out_of_place": rounds(lambda: _check(lib.ibu_records_swap_umi_index(ctx._c, _dptr(orig), _dptr(d), n, st)))}
        merge(None)
        ctx.synchronize(st)
        assert ctx.is_sorted(d, n)
        res["sort_of_concatenation"] = rounds(lambda: _check(lib.ibu_sort_records(ctx._c, _dptr(d), _dptr(t), n, st)), before=restore)
        res["merge_over_copy"] = round(res["merge"]["median_ms"] / res["copy"]["median_ms"], 3)
        res["merge_over_sort"] = round(res["merge"]["median_ms"] / res["sort_of_concatenation"]["median_ms"], 3)
        return res

    out = {"n": n, "lens": [bc_len, umi_len], "rounds": a.rounds, "two_way": {}, "runs": {}}
    random_records()
    out["two_way"]["interleaved"] = two_way("interleaved")
    out["two_way"]["disjoint"] = two_way("disjoint")
    whitelist_records()
    out["two_way"]["whitelist"] = two_way("whitelist")
    for k in (2, 8, 64):
        random_records()
        sort_runs(k)
        lengths = (C.c_size_t * k)(*[n // k] * k)
        r = {"merge_runs": rounds(lambda: _check(lib.ibu_merge_sorted_runs(ctx._c, _dptr(d), _dptr(t), lengths, k, st)), before=restore)}
        ctx.synchronize(st)
        assert ctx.is_sorted(d, n)
        r["sort_of_concatenation"] = rounds(lambda: _check(lib.ibu_sort_records(ctx._c, _dptr(d), _dptr(t), n, st)), before=restore)
        r["levels"] = (k - 1).bit_length()
        r["merge_runs_over_sort"] = round(r["merge_runs"]["median_ms"] / r["sort_of_concatenation"]["median_ms"], 3)
        out["runs"][str(k)] = r
    print(json.dumps(out), flush=True)
    for b in (orig, d, t, src):
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default=None, help="comma list (default 1e8; with --merge one value, default 1e9)")
    ap.add_argument("--merge", action="store_true",
                    help="time ibu_merge_sorted / ibu_merge_sorted_runs beside the copy, the field exchange and the sort on the same arrays")
    ap.add_argument("--lens", default="16,12")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--random-index", action="store_true",
                    help="index column in random order (default: increasing = records in read order, whose index passes are skipped)")
    ap.add_argument("--variants", default="0", help="comma list of sort_variant values to time (A/B in one process)")
    ap.add_argument("--compact", default="", help="comma list of sort_compact values to time (0 = 24-byte passes only, k = compact tile shape k; "
                                                  "default: the library's default)")
    ap.add_argument("--skip-agg", action="store_true")
    ap.add_argument("--guess", default="", help="comma list of sort_guess values to time (1 = the library default: speculation from 2^23 records; k = from k records)")
    ap.add_argument("--hybrid", default="", help="comma list of sort_hybrid values (0 = all passes, 1 = default)")
    ap.add_argument("--whitelist", type=int, default=0,
                    help="K > 0: barcodes drawn from K distinct ones with a skewed distribution (rank ~ K u^3: a single-cell run, where a few "
                         "thousand cells hold most reads), random UMIs, records in read order; built on the device with torch")
    ap.add_argument("--sort-first", action="store_true", help="with --shards: force the round-3 form of ibu_sort_records_contexts (sort_compact = 0 on the first context)")
    ap.add_argument("--shards", type=int, default=0,
                    help="K > 0: time ibu_sort_records_contexts over K contexts instead — all on device 0 (the one-GPU rehearsal of the "
                         "multi-GPU sort: K local sorts, the device-to-device exchange, K sorts of what arrived), n / K records each")
    ap.add_argument("--presorted", action="store_true", help="also time ibu_sort_records on the SORTED result (the already-sorted fast exit: one read-only census)")
    a = ap.parse_args()
    if a.merge:
        return merge_main(a)
    a.records = a.records or "1e8"
    if a.whitelist:
        import torch                                         # before the library, as bench.py does: its HIP runtime is the process's
        torch.cuda.init()
    import ibu_amd as ia

    bc_len, umi_len = (int(x) for x in a.lens.split(","))
    if a.shards:
        return shards_main(a, ia, bc_len, umi_len)
    ctx = ia.Context(0)
    for n in (int(float(x)) for x in a.records.split(",")):
        d, t = ctx.alloc(24 * n), ctx.alloc(24 * n)
        cols = [ctx.alloc(8 * n) for _ in range(4)] if (a.random_index or a.whitelist) else None
        if a.whitelist:
            g = torch.Generator(device="cuda").manual_seed(0x1B00007)
            wl = _rand_bits(torch, g, 2 * bc_len, a.whitelist)
            bc, um, ix = (torch.as_tensor(c, device="cuda").view(torch.int64) for c in cols[:3])
            step = 1 << 26
            for lo in range(0, n, step):                     # in pieces: the temporaries stay small
                hi = min(n, lo + step)
                u = torch.rand(hi - lo, generator=g, device="cuda", dtype=torch.float64)
                bc[lo:hi] = wl[(u * u * u * a.whitelist).to(torch.int64).clamp_(max=a.whitelist - 1)]
                um[lo:hi] = _rand_bits(torch, g, 2 * umi_len, hi - lo)
                ix[lo:hi] = (torch.randint(0, 1 << 30, (hi - lo,), generator=g, device="cuda", dtype=torch.int64) if a.random_index
                             else torch.arange(lo, hi, device="cuda", dtype=torch.int64))
            del u
            torch.cuda.synchronize()
        for variant, compact, guess, hybrid in ((int(v), c, g, h) for v in a.variants.split(",") for c in (a.compact.split(",") if a.compact else [None])
                                                for g in (a.guess.split(",") if a.guess else [None]) for h in (a.hybrid.split(",") if a.hybrid else [None])):
            ctx.set_option("sort_variant", variant)
            if guess is not None:
                ctx.set_option("sort_guess", int(guess))
            if hybrid is not None:
                ctx.set_option("sort_hybrid", int(hybrid))
            if compact is not None:
                ctx.set_option("sort_compact", int(compact))
            ts = []
            for _ in range(a.rounds + 1):
                if a.whitelist:
                    ctx.serialize(cols[0], cols[1], cols[2], n, d)
                else:
                    ctx.generate(0x1B00005, 0, n, bc_len, umi_len, d)  # random barcode/UMI, increasing index: unsorted
                if a.random_index and not a.whitelist:  # replace the index column by random 30-bit values (another stream's barcode column)
                    ctx.deserialize(d, n, cols[0], cols[1], cols[2])
                    ctx.generate(0x1B00006, 0, n, 15, 1, t)
                    ctx.deserialize(t, n, cols[3], cols[2], cols[2])
                    ctx.serialize(cols[0], cols[1], cols[3], n, d)
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.sort_records(d, t, n)
                ctx.synchronize()
                ts.append(time.perf_counter() - t0)
            assert os.environ.get("IBU_HIP_SO") or ctx.is_sorted(d, n)  # probe builds (IBU_HIP_SO=...): wrong output by design; variants >= 4 exist in probe builds only: wrong output by design
            agg, nb = None, None
            if not a.skip_agg:
                t0 = time.perf_counter()
                bcs, counts, uniq = ctx.barcode_counts(d, n)  # BarcodeAnalyzer on the sorted records (size query + emit + download)
                agg = round(time.perf_counter() - t0, 4)
                assert int(counts.sum()) == n
                nb = int(len(bcs))
            presorted = None
            if a.presorted:
                tp = []
                for _ in range(a.rounds + 1):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    ctx.sort_records(d, t, n)
                    ctx.synchronize()
                    tp.append(time.perf_counter() - t0)
                presorted = round(statistics.median(tp[1:]) * 1e3, 3)
            sec = statistics.median(ts[1:])
            idx_bytes = 4 if a.random_index else 0  # 30 random bits -> 4 digit passes; index-ordered input -> skipped
            passes = (2 * bc_len + 7) // 8 + (2 * umi_len + 7) // 8 + idx_bytes
            # algorithmic traffic: census 24 + histogram 24 once, 48 per pass, 48 for the copy back after an odd number of passes
            alg = n * (48 + 48 * passes + (48 if passes & 1 else 0))
            print(json.dumps({"n": n, "lens": [bc_len, umi_len], "variant": variant, "compact": compact if compact is None else int(compact), "guess": guess, "hybrid": hybrid, "index": "random" if a.random_index else "increasing (read order)", "whitelist": a.whitelist or None,
                              "seconds": round(sec, 4), "best": round(min(ts[1:]), 4), "M_records_per_s": round(n / sec / 1e6, 1),
                              "passes": passes, "presorted_input_ms": presorted, "barcode_counts_seconds": agg, "distinct_barcodes": nb,
                              "algorithmic_GB": round(alg / 1e9, 1), "GBps_algorithmic": round(alg / sec / 1e9)}), flush=True)
        d.free()
        t.free()
        for c in cols or []:
            c.free()


if __name__ == "__main__":
    main()
