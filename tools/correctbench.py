#!/usr/bin/env python3
"""Barcode correction against a whitelist on device-resident records: ibu_correct_barcodes (with class bytes) timed against
ibu_reduce — the library's plain 24-bytes-read-per-record kernel — in the same process, on the same array, interleaved; and
ibu_select_records (classes 0 | 1) against ibu_device_copy of the bytes it keeps.  One JSON line per configuration.
  python tools/correctbench.py [--records 1e9] [--whitelists 1e5,1e6,6.9e6] [--errors 0,0.02,0.1] [--random 0.01] [--rounds 5]
Barcodes of 16 bases drawn uniformly from the whitelist; `errors` of them get one substituted base, `random` of them (1 % unless
told otherwise; 0 leaves the hit path alone) are uniform random.
Times are HIP events on the stream the calls run on (the select call synchronises once inside: its time includes that).
  python tools/correctbench.py --resolve [--records 1e9] [--whitelists 1e5,6.9e6] [--errors 0.02] [--rounds 5]
A leg of its own (the lines above are not printed): the resolution of ambiguous barcodes.  Per configuration, in one process on one
array: ibu_reduce (the plain 24-byte read), ibu_device_copy of the array, ibu_correct_barcodes, ibu_abundance_add over the class-0
records in read order, the same add without class bytes in read order and on the same records SORTED (what run merging is for),
and ibu_resolve_barcodes at 39/40.
  python tools/correctbench.py --labels [--records 1e9] [--whitelists 1e5] [--errors 0.02] [--rounds 5]
A leg of its own on the same arrays: per-barcode labels onto records.  Per configuration, in one process on one array and one
whitelist (entry of rank r labelled r % 256), in read order and then on the same records SORTED: ibu_reduce (the plain 24-byte read),
ibu_correct_barcodes(max_mismatches=0) with class bytes — the yardstick: the same read, one probe and a 1-byte write — and
ibu_label_records with class bytes, with class bytes and the histogram, and with the histogram alone.
  python tools/correctbench.py --partition [--records 1e9] [--whitelists 1e5] [--errors 0.02] [--rounds 5]
A leg of its own on the same arrays: the multi-way partition by class byte.  Per configuration, in read order and then on the same
records SORTED: ibu_device_copy of the array and ibu_select_records keeping every record of it (a class array of zeros) — the
yardsticks: the same reads, the same 24-byte writes, the same unit walk — and, for S = 2, 8, 16 and 255 labels dealt evenly over the
whitelist, ibu_partition_records on the class bytes of ibu_label_records in plain mode: the size query (count + scan) and the whole
call, each with its one synchronisation inside; scatter_ms is the difference of the two medians.  For S = 8 also the chain the one
call replaces: eight ibu_label_records(match) + ibu_select_records pairs, whose counts and record checksums must equal the parts."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="1e9")
    ap.add_argument("--whitelists", default="1e5,1e6,6.9e6")
    ap.add_argument("--errors", default="0,0.02,0.1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--random", type=float, default=0.01, help="share of uniform random barcodes (they always take the miss path)")
    ap.add_argument("--resolve", action="store_true", help="the abundance / resolve leg instead of the correct / select one")
    ap.add_argument("--labels", action="store_true", help="the label leg instead of the correct / select one")
    ap.add_argument("--partition", action="store_true", help="the partition leg instead of the correct / select one")
    a = ap.parse_args()
    import torch                                             # before the library, as bench.py does
    torch.cuda.init()
    import ibu_amd as ia

    bc_len, umi_len = 16, 12
    ctx = ia.Context(0)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    n = int(float(a.records))
    asked = n
    while True:                                              # fall back to half the records if memory is short, and say so
        try:
            d, orig, out, d_cls = ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(24 * n), ctx.alloc(n)
            cols = [ctx.alloc(8 * n) for _ in range(3)]
            break
        except ia.IbuError:
            for b in list(ctx._buffers):
                b.free()
            n //= 2
            if n < 1000:
                raise
    g = torch.Generator(device="cuda").manual_seed(0x1B00008)
    ctx.generate(0x1B00005, 0, n, bc_len, umi_len, orig)
    ctx.deserialize(orig, n, cols[0], cols[1], cols[2])
    ctx.synchronize()
    bc = torch.as_tensor(cols[0], device="cuda").view(torch.int64)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stat(v):
        v = v[1:]                                            # the first round is the warm-up
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    for w in (int(float(x)) for x in a.whitelists.split(",")):
        codes = torch.unique(torch.randint(0, 1 << (2 * bc_len), (w + w // 64 + 1024,), generator=g, device="cuda", dtype=torch.int64))
        codes = codes[torch.randperm(len(codes), generator=g, device="cuda")][:w].contiguous()
        torch.cuda.synchronize()
        wl = ia.Whitelist(ctx, codes, len(codes), bc_len)
        for err in (float(x) for x in a.errors.split(",")):
            for lo in range(0, n, 1 << 26):
                hi = min(n, lo + (1 << 26))
                k = hi - lo
                b = codes[torch.randint(0, len(codes), (k,), generator=g, device="cuda", dtype=torch.int64)]
                u = torch.rand(k, generator=g, device="cuda")
                flip = torch.randint(1, 4, (k,), generator=g, device="cuda", dtype=torch.int64) << (2 * torch.randint(0, bc_len, (k,), generator=g, device="cuda", dtype=torch.int64))
                b = torch.where(u < err, b ^ flip, b)
                b = torch.where(u >= 1.0 - a.random, torch.randint(0, 1 << (2 * bc_len), (k,), generator=g, device="cuda", dtype=torch.int64), b)
                bc[lo:hi] = b
            del b, u, flip
            torch.cuda.synchronize()
            ctx.serialize(cols[0], cols[1], cols[2], n, orig)
            ctx.synchronize()
            if a.resolve:
                resolve_leg(ia, ctx, st, timed, stat, wl, d, orig, out, d_cls, n, asked, bc_len, len(codes), err, a)
                continue
            if a.labels:
                labels_leg(ia, ctx, torch, st, timed, stat, wl, codes, d, orig, out, d_cls, n, asked, bc_len, err, a)
                continue
            if a.partition:
                partition_leg(ia, ctx, torch, st, timed, stat, wl, codes, d, orig, out, d_cls, n, asked, bc_len, err, a)
                continue
            t_red, t_cor, t_sel, t_cpy = [], [], [], []
            counts = kept = None
            k_out = C.c_size_t()
            for _ in range(a.rounds + 1):
                ctx.copy(d, orig, 24 * n, stream=st)
                t_red.append(timed(lambda: ctx.reduce(d, n, stream=st, reset=False, fetch=False)))
                t_cor.append(timed(lambda: ctx.correct_barcodes(wl, d, n, 1, d_cls, counts=False, stream=st)))
                t_sel.append(timed(lambda: ia._check(ia.lib.ibu_select_records(ctx._c, d.ptr, d_cls.ptr, n, 0b0011, out.ptr, n, C.byref(k_out), st))))
                kept = k_out.value
                t_cpy.append(timed(lambda: ctx.copy(out, d, 24 * kept, stream=st)))
            ctx.copy(d, orig, 24 * n, stream=st)
            counts = ctx.correct_barcodes(wl, d, n, 1, d_cls, stream=st)
            red, cor, sel, cpy = stat(t_red), stat(t_cor), stat(t_sel), stat(t_cpy)
            print(json.dumps({"n": n, "records_asked": asked, "bc_len": bc_len, "w": len(codes), "table_MiB": round(wl.device_bytes / 2**20, 1),
                              "errors": err, "random": a.random, "counts": counts, "kept": kept,
                              "reduce": red, "correct": cor, "correct_over_reduce": round(cor["median_ms"] / red["median_ms"], 3),
                              "correct_GBps_of_25B": round(25 * n / cor["median_ms"] / 1e6),
                              "select": sel, "copy_of_kept": cpy, "select_over_copy": round(sel["median_ms"] / cpy["median_ms"], 3)}), flush=True)
        wl.close()
    ctx.close()


def resolve_leg(ia, ctx, st, timed, stat, wl, d, orig, out, d_cls, n, asked, bc_len, w, err, a):
    t = {k: [] for k in ("reduce", "copy", "correct", "add_read_order", "add_read_order_no_class", "add_sorted_no_class", "resolve")}
    ab = wl.abundance()
    for _ in range(a.rounds + 1):
        ctx.copy(d, orig, 24 * n, stream=st)
        t["reduce"].append(timed(lambda: ctx.reduce(d, n, stream=st, reset=False, fetch=False)))
        t["copy"].append(timed(lambda: ctx.copy(out, d, 24 * n, stream=st)))
        t["correct"].append(timed(lambda: ctx.correct_barcodes(wl, d, n, 1, d_cls, counts=False, stream=st)))
        ab.reset(stream=st)
        t["add_read_order_no_class"].append(timed(lambda: ab.add(d, n, stream=st)))
        ab.reset(stream=st)
        t["add_read_order"].append(timed(lambda: ab.add(d, n, d_cls, 1, stream=st)))
        t["resolve"].append(timed(lambda: ctx.resolve_barcodes(wl, ab, d, n, d_cls, counts=False, stream=st)))
    ctx.copy(d, orig, 24 * n, stream=st)
    counts = ctx.correct_barcodes(wl, d, n, 1, d_cls, stream=st)
    ab.reset(stream=st)
    ab.add(d, n, d_cls, 1, stream=st)
    totals = ctx.resolve_barcodes(wl, ab, d, n, d_cls, stream=st)
    ab.reset(stream=st)
    ab.add(d, n, stream=st)                                  # what the sorted add must reproduce: the whitelist hits after correct and resolve
    ctx.synchronize(st)
    probe = ia.DeviceBuffer.wrap(ctx, d.ptr, 8 * 3 * min(n, 4096)).download("<u8")[::3] & ((1 << (2 * bc_len)) - 1)   # the first 4096 barcodes
    before = ab.counts(probe, stream=st)
    ctx.copy(out, d, 24 * n, stream=st)
    ctx.sort_records(out, d, n, stream=st)                   # d is scratch from here on
    for _ in range(a.rounds + 1):
        ab.reset(stream=st)
        t["add_sorted_no_class"].append(timed(lambda: ab.add(out, n, stream=st)))
    same = bool((ab.counts(probe, stream=st) == before).all())
    hits = counts["exact"] + counts["corrected"] + totals["resolved"]
    s = {k: stat(v) for k, v in t.items()}
    ms = {k: v["median_ms"] for k, v in s.items()}
    print(json.dumps({"leg": "resolve", "n": n, "records_asked": asked, "bc_len": bc_len, "w": w, "table_MiB": round(wl.device_bytes / 2**20, 1),
                      "counters_MiB": round(ab.device_bytes / 2**20, 1), "errors": err, "random": a.random, "counts": counts, "resolve_totals": totals,
                      "share": [39, 40], **s,
                      "add_over_correct": round(ms["add_read_order"] / ms["correct"], 3),
                      "add_no_class_over_correct": round(ms["add_read_order_no_class"] / ms["correct"], 3),
                      "add_sorted_over_correct": round(ms["add_sorted_no_class"] / ms["correct"], 3),
                      "resolve_over_correct": round(ms["resolve"] / ms["correct"], 3),
                      "correct_over_reduce": round(ms["correct"] / ms["reduce"], 3),
                      "atomics_per_s_read_order": round(counts["exact"] / ms["add_read_order"] * 1e3),
                      "atomics_per_s_read_order_no_class": round(hits / ms["add_read_order_no_class"] * 1e3),
                      "sorted_counters_equal_read_order": same}), flush=True)
    ab.close()


def labels_leg(ia, ctx, torch, st, timed, stat, wl, codes, d, orig, out, d_cls, n, asked, bc_len, err, a):
    calls = ("reduce", "correct0", "label_class", "label_class_hist", "label_hist")
    w = len(codes)
    unsigned = codes ^ torch.iinfo(torch.int64).min          # int64 order of this = unsigned order of the codes (32 bases set the top bit)
    labs = (torch.argsort(torch.argsort(unsigned)) % 256).to(torch.uint8).contiguous()   # rank % 256
    torch.cuda.synchronize()
    lb = wl.labels(fill=255)
    ia._check(ia.lib.ibu_labels_set(ctx._c, lb._c, codes.data_ptr(), labs.data_ptr(), w, None, None))
    ctx.synchronize()
    result = {"leg": "labels", "n": n, "records_asked": asked, "bc_len": bc_len, "w": w, "table_MiB": round(wl.device_bytes / 2**20, 1),
              "labels_MiB": round(lb.device_bytes / 2**20, 2), "errors": err, "random": a.random}
    hists = {}
    for order in ("read_order", "sorted"):
        if order == "read_order":
            ctx.copy(d, orig, 24 * n, stream=st)
            recs = d
        else:
            ctx.copy(out, orig, 24 * n, stream=st)
            ctx.sort_records(out, d, n, stream=st)               # d is scratch from here on
            recs = out
        t = {k: [] for k in calls}
        for _ in range(a.rounds + 1):
            t["reduce"].append(timed(lambda: ctx.reduce(recs, n, stream=st, reset=False, fetch=False)))
            t["correct0"].append(timed(lambda: ctx.correct_barcodes(wl, recs, n, 0, d_cls, counts=False, stream=st)))
            t["label_class"].append(timed(lambda: ctx.label_records(lb, recs, n, d_class=d_cls, stream=st)))
            t["label_class_hist"].append(timed(lambda: ctx.label_records(lb, recs, n, d_class=d_cls, hist=True, stream=st)))
            t["label_hist"].append(timed(lambda: ctx.label_records(lb, recs, n, hist=True, stream=st)))
        hists[order] = ctx.label_records(lb, recs, n, hist=True, stream=st)
        s = {k: stat(v) for k, v in t.items()}
        ms = {k: v["median_ms"] for k, v in s.items()}
        result[order] = {**s, "correct0_over_reduce": round(ms["correct0"] / ms["reduce"], 3),
                         **{k + "_over_correct0": round(ms[k] / ms["correct0"], 3) for k in calls[2:]}}
    result["found"] = int(hists["read_order"][:256].sum())
    result["not_found"] = int(hists["read_order"][256])
    result["sorted_histogram_equals_read_order"] = bool((hists["read_order"] == hists["sorted"]).all()) and int(hists["sorted"].sum()) == n
    print(json.dumps(result), flush=True)
    lb.close()


def partition_leg(ia, ctx, torch, st, timed, stat, wl, codes, d, orig, out, d_cls, n, asked, bc_len, err, a):
    w = len(codes)
    unsigned = codes ^ torch.iinfo(torch.int64).min          # int64 order of this = unsigned order of the codes
    rank = torch.argsort(torch.argsort(unsigned))
    zeros = torch.zeros(n, dtype=torch.uint8, device="cuda")  # the class array of the select that keeps everything
    torch.cuda.synchronize()
    lb = wl.labels(fill=255)
    result = {"leg": "partition", "n": n, "records_asked": asked, "bc_len": bc_len, "w": w, "errors": err, "random": a.random}
    k_out = C.c_size_t()

    def select(src, cls_ptr, mask, dst, cap):
        ia._check(ia.lib.ibu_select_records(ctx._c, src.ptr, cls_ptr, n, mask, dst.ptr if dst is not None else None, cap, C.byref(k_out), st))
        return k_out.value

    def partition(src, parts, dst, offsets):
        ia._check(ia.lib.ibu_partition_records(ctx._c, src.ptr, d_cls.ptr, n, None, parts, dst.ptr if dst is not None else None, n if dst is not None else 0,
                                               offsets, st))

    for order in ("read_order", "sorted"):
        if order == "read_order":
            ctx.copy(d, orig, 24 * n, stream=st)
            recs, dst = d, out
        else:
            ctx.copy(out, orig, 24 * n, stream=st)
            ctx.sort_records(out, d, n, stream=st)               # d is the destination from here on
            recs, dst = out, d
        t = {"copy": [], "select_all_query": [], "select_all": []}
        for _ in range(a.rounds + 1):
            t["copy"].append(timed(lambda: ctx.copy(dst, recs, 24 * n, stream=st)))
            t["select_all_query"].append(timed(lambda: select(recs, zeros.data_ptr(), 1, None, 0)))
            t["select_all"].append(timed(lambda: select(recs, zeros.data_ptr(), 1, dst, n)))
        assert k_out.value == n
        res = {k: stat(v) for k, v in t.items()}
        sel = res["select_all"]["median_ms"]
        for parts in (2, 8, 16, 255):
            labs = (rank % parts).to(torch.uint8).contiguous()
            torch.cuda.synchronize()
            ia._check(ia.lib.ibu_labels_set(ctx._c, lb._c, codes.data_ptr(), labs.data_ptr(), w, None, st))
            tl, tq, tp = [], [], []
            offsets = (C.c_uint64 * (parts + 1))()
            for _ in range(a.rounds + 1):
                tl.append(timed(lambda: ctx.label_records(lb, recs, n, d_class=d_cls, stream=st)))
                tq.append(timed(lambda: partition(recs, parts, None, offsets)))
                tp.append(timed(lambda: partition(recs, parts, dst, offsets)))
            off = list(offsets)
            r = {"label_plain": stat(tl), "query": stat(tq), "partition": stat(tp), "kept": off[parts]}
            r["scatter_ms"] = round(r["partition"]["median_ms"] - r["query"]["median_ms"], 3)
            r["partition_over_select_all"] = round(r["partition"]["median_ms"] / sel, 3)
            r["partition_over_copy"] = round(r["partition"]["median_ms"] / res["copy"]["median_ms"], 3)
            if parts == 8:                                       # the chain the one call replaces; its outputs land in the columns' memory
                ctx.synchronize(st)
                sums = [ctx.reduce(ia.DeviceBuffer.wrap(ctx, dst.ptr + 24 * off[p], 24 * (off[p + 1] - off[p])), off[p + 1] - off[p]) for p in range(parts)]
                tc, same = [], True
                for rnd in range(a.rounds + 1):
                    def chain():
                        nonlocal same
                        for p in range(parts):
                            ctx.label_records(lb, recs, n, d_class=d_cls, match=p, stream=st)
                            k = select(recs, d_cls.ptr, 1 << ia.LABEL_IS, dst, n)
                            if rnd == 0:                         # (the warm-up round: checked, not timed)
                                ctx.synchronize(st)
                                same = same and k == off[p + 1] - off[p] and ctx.reduce(dst, k) == sums[p]
                    tc.append(timed(chain))
                r["chain_of_8_label_select_pairs"] = stat(tc)
                r["chain_equals_partition"] = same
                r["chain_over_label_plus_partition"] = round(r["chain_of_8_label_select_pairs"]["median_ms"] /
                                                             (r["label_plain"]["median_ms"] + r["partition"]["median_ms"]), 3)
                ctx.label_records(lb, recs, n, d_class=d_cls, stream=st)   # the class bytes of the plain mode again
            res[f"S{parts}"] = r
        result[order] = res
    print(json.dumps(result), flush=True)
    lb.close()


if __name__ == "__main__":
    main()
