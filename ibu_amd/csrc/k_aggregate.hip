// k_aggregate.hip — run-length aggregation of SORTED records: the device form of the reference's BarcodeAnalyzer processor
// (src/parallel.rs:72-98: HashMap<barcode, count> merged in on_batch_complete).  On sorted input a barcode is a run, so the map is a
// run-length encoding: barcodes[k], counts[k] and — the UMI-dedup figure single-cell pipelines want from exactly this layout —
// unique_umis[k] = number of distinct (barcode, umi) pairs in the run.  Output order = ascending barcode (the map's sorted keys).
// ibu_pair_counts is the same one level deeper: runs of equal (w0, w1), the distinct (w0, w1, w2) counted inside them.
//
// Two passes over the segments of runs_walk.hpp, one wave each.  The count pass (ibu_k_runs_count, _count_stash, ibu_k_pairs_count)
// leaves run heads and ranked heads per segment in a [2][nseg] table, ibu_k_runs_scan turns it into bases and the two totals, which
// go back to the host to size the output.  The emit pass (ibu_k_runs_emit, ibu_k_pairs_emit) walks again and writes each run's key,
// first record and rank with plain stores, and ibu_k_runs_finish turns neighbouring entries into counts (no atomics anywhere: the
// first version used two per run and took 1 s on 0.9e9 runs of length one).
//
// ONE read of the records where barcode runs are long: ibu_k_runs_count_stash also keeps the first kStashHeads run heads of every
// segment (barcode, row inside the segment, pair rank inside the segment: 16 bytes each, plain stores — there are few) in the scratch;
// ibu_k_runs_emit serves a segment with that many heads or fewer FROM THE STASH (a few lanes, no record read) and walks only the
// others again.  Whitelist barcodes (1e5 runs in 1e9 records, 0.8 heads per segment): 24 B/record instead of 48; every record its own
// barcode: as before.  The pair level has no stash: entries are typically a sizeable fraction of the records (a count matrix has a few
// reads per entry), and a segment with more than kStashHeads of them is walked again anyway.
//
// ibu_k_class_fill: the pass that turns the ballots a walk kept into class bytes, for the molecule classification (k_molecules.hip,
// on the pair-level count pass) and cell calling (k_cells.hip, on the barcode-level one).
//
// Launchers: launch_runs_count, launch_runs_emit, launch_class_fill (kernels.h); C ABI: ibu_barcode_counts, ibu_pair_counts (api_analysis.cpp).
#include "runs_walk.hpp"

namespace ibu {

// ---- the sinks (NoSink, runs_walk.hpp) ----
struct StashSink : NoSink {                                 // the segment's first run heads, ranks counted from the segment's start
  RunStash* mine; u64 row0;
  __device__ __forceinline__ void head(u64 k, u64 q, u64 row, u64 b, u64, bool run_head) const {
    if (run_head && k < kStashHeads) { RunStash e; e.barcode = b; e.row_off = (u32)(row - row0); e.pair_local = (u32)q; mine[k] = e; }
  }
};
struct BarcodeEmit : NoSink {
  u64* barcodes; u64* starts; u64* pair_rank /*nullable*/;
  __device__ __forceinline__ void head(u64 k, u64 q, u64 row, u64 b, u64, bool run_head) const {
    if (!run_head) return;
    barcodes[k] = b;
    starts[k] = row;                                        // first record of run k
    if (pair_rank) pair_rank[k] = q;                        // (barcode, umi) pairs that start before it
  }
};
struct PairEmit : NoSink {
  u64* first; u64* second; u64* starts; u64* triple_rank /*nullable*/;
  __device__ __forceinline__ void head(u64 k, u64 q, u64 row, u64 w0, u64 w1, bool run_head) const {
    if (!run_head) return;
    first[k] = w0;
    second[k] = w1;
    starts[k] = row;                                        // first record of entry k
    if (triple_rank) triple_rank[k] = q;                    // (w0, w1, w2) heads in front of it
  }
};

extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_runs_count(const u64* __restrict__ recs, SegPlan sp, u32* __restrict__ seg_heads /*[2][nseg]*/) {
  runs_kernel<1>(recs, sp, nullptr, seg_heads, NoSink{});
}
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_runs_count_stash(const u64* __restrict__ recs, SegPlan sp, u32* __restrict__ seg_heads /*[2][nseg]*/, RunStash* __restrict__ stash /*[nseg][kStashHeads]*/) {
  const u32 seg = wave_segment();
  runs_kernel<1>(recs, sp, nullptr, seg_heads, StashSink{{}, stash + (size_t)seg * kStashHeads, seg_first_row(sp, seg)});
}
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_runs_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/,
                const u32* __restrict__ seg_heads /*[2][nseg]*/, const RunStash* __restrict__ stash /*[nseg][kStashHeads]*/,
                u64* __restrict__ barcodes, u64* __restrict__ starts, u64* __restrict__ pair_rank) {
  const u32 lane = threadIdx.x & (kWave - 1), seg = wave_segment();
  if (seg >= sp.nseg) return;
  const u32 heads = seg_heads[seg];
  if (heads <= kStashHeads) {                               // wave-uniform: the heads the count pass kept are all of them
    if (lane < heads) {
      const RunStash e = stash[(size_t)seg * kStashHeads + lane];
      const u64 k = seg_base[seg] + lane;
      barcodes[k] = e.barcode;
      starts[k] = seg_first_row(sp, seg) + e.row_off;
      if (pair_rank) pair_rank[k] = seg_base[sp.nseg + seg] + e.pair_local;
    }
    return;
  }
  runs_kernel<1>(recs, sp, seg_base, nullptr, BarcodeEmit{{}, barcodes, starts, pair_rank});
}
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_pairs_count(const u64* __restrict__ recs, SegPlan sp, u32* __restrict__ seg_heads /*[2][nseg]*/) {
  runs_kernel<2>(recs, sp, nullptr, seg_heads, NoSink{});
}
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_pairs_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/,
                 u64* __restrict__ first, u64* __restrict__ second, u64* __restrict__ starts, u64* __restrict__ triple_rank) {
  runs_kernel<2>(recs, sp, seg_base, nullptr, PairEmit{{}, first, second, starts, triple_rank});
}
// counts[k] = start(k+1) - start(k), unique_umis[k] = pair_rank(k+1) - pair_rank(k); entry n_runs is the sentinel.
extern "C" __global__ void ibu_k_runs_finish(const u64* __restrict__ starts, const u64* __restrict__ pair_rank, u64 n_runs, u64 n,
                                             u64 n_pairs, u64* __restrict__ counts, u64* __restrict__ uniq) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < n_runs; k += stride) {
    counts[k] = closed_diff(starts, k, n_runs, n);
    if (uniq) uniq[k] = closed_diff(pair_rank, k, n_runs, n_pairs);
  }
}

// seg_heads u32 [2][nseg] -> seg_base u64 [2][nseg] (exclusive prefix per row) and the two row totals.  One workgroup per row;
// u64 sums: 2^32 or more records (and then possibly 2^32 or more runs) fit in 288 GB.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_runs_scan(const u32* __restrict__ seg_heads, u32 nseg, u64* __restrict__ seg_base, u64* __restrict__ totals) {
  __shared__ u32 wsum[kSortWaves];
  const u32* row = seg_heads + (size_t)blockIdx.x * nseg;
  u64* out = seg_base + (size_t)blockIdx.x * nseg;
  u64 carry = 0;
  for (u32 base = 0; base < nseg; base += 4 * kSortThreads) {   // 1024 segments per round: at most 2^23 heads, fits u32
    const u32 i0 = base + 4 * threadIdx.x;
    u32 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i0 + j < nseg ? row[i0 + j] : 0;
    u32 tot;
    u32 ex = block_exclusive_scan(v[0] + v[1] + v[2] + v[3], wsum, &tot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < nseg) out[i0 + j] = carry + ex;
      ex += v[j];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Class bytes from the ballots an emit pass kept (BallotSink, runs_walk.hpp): the heads' ordinals are the entries of `verdict`.  One
// wave per segment, as in the walk; in a tiled segment lane L first takes tile L's two ballots and the wave ranks the tiles, then every
// step serves two tiles: lanes 0-31 the first, lanes 32-63 the second, four consecutive records (two even, two odd positions of the
// walk's lane pairs) per lane.  A record's entry = the heads that begin in front of the segment (seg_row: the scanned row of seg_base
// that counts these heads) + the heads of the segment up to and including the record - 1: a record whose run began in an earlier
// segment falls out of the same formula.  No record read, no LDS.
template <bool WORDS>
__global__ void __launch_bounds__(kSortThreads)
ibu_k_class_fill(SegPlan sp, const u64* __restrict__ seg_row /*[nseg], scanned*/, const u64* __restrict__ masks,
                 const uint8_t* __restrict__ verdict, uint8_t* __restrict__ d_class) {
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;                                 // wave-uniform
  const u64 hbase = seg_row[seg];                             // heads that begin in front of the segment
  const u64 ntiles_all = sp.main / kTileRecs;
  if (seg == 0 || seg == sp.nseg - 1) {
    const u64 begin = seg == 0 ? 0 : sp.head + sp.main, end = seg == 0 ? sp.head : sp.n;
    u64 seen = 0;
    for (u32 step = 0; step < 2; ++step) {
      const u64 i = begin + (u64)step * kWave + lane;
      if (begin + (u64)step * kWave >= end) break;             // wave-uniform
      const u64 m = masks[end_ballots_at(ntiles_all, seg == 0 ? 0 : 1, step)];
      if (i < end) d_class[i] = verdict[hbase + seen + (u64)__popcll(m & ((2ull << lane) - 1)) - 1];
      seen += (u64)__popcll(m);
    }
    return;
  }
  const u64 begin = sp.head + (u64)(seg - 1) * kSegRecs, stop = sp.head + sp.main;
  const u32 ntiles = (u32)(((begin + kSegRecs < stop ? begin + kSegRecs : stop) - begin) / kTileRecs);   // 1 .. 64
  const u64 tile0 = (begin - sp.head) / kTileRecs;
  u64 even = 0, odd = 0;
  if (lane < ntiles) { even = masks[tile_ballots_at(tile0 + lane)]; odd = masks[tile_ballots_at(tile0 + lane) + 1]; }
  const u32 mine = (u32)(__popcll(even) + __popcll(odd));
  const u32 rank = wave_scan(mine, OpAdd{}) - mine;           // heads that begin in the segment's tiles in front of tile `lane`
  const u32 l = lane & 31u;
  const u64 below = (1ull << (2 * l)) - 1;
  for (u32 step = 0; 2 * step < ntiles; ++step) {
    const u32 tile = 2 * step + (lane >> 5);
    const u64 ev = ((u64)__shfl((u32)(even >> 32), tile) << 32) | __shfl((u32)even, tile);
    const u64 od = ((u64)__shfl((u32)(odd >> 32), tile) << 32) | __shfl((u32)odd, tile);
    const u32 r0 = __shfl(rank, tile);
    if (tile < ntiles) {
      // records 4l .. 4l+3 of the tile = the walk's (lane 2l: even, odd), (lane 2l+1: even, odd)
      const u64 k0 = hbase + r0 + (u64)(__popcll(ev & below) + __popcll(od & below)) + ((ev >> (2 * l)) & 1) - 1;
      const u64 k1 = k0 + ((od >> (2 * l)) & 1);
      const u64 k2 = k1 + ((ev >> (2 * l + 1)) & 1);
      const u64 k3 = k2 + ((od >> (2 * l + 1)) & 1);
      const u32 v0 = verdict[k0], v1 = verdict[k1], v2 = verdict[k2], v3 = verdict[k3];
      uint8_t* out = d_class + begin + (u64)tile * kTileRecs + 4 * l;
      if constexpr (WORDS) {
        __builtin_nontemporal_store(v0 | (v1 << 8) | (v2 << 16) | (v3 << 24), reinterpret_cast<u32*>(out));
      } else {
        out[0] = (uint8_t)v0; out[1] = (uint8_t)v1; out[2] = (uint8_t)v2; out[3] = (uint8_t)v3;
      }
    }
  }
}

void launch_runs_scan(const u32* seg_heads, u32 nseg, u32 rows, u64* seg_base, u64* totals, hipStream_t st) {
  hipLaunchKernelGGL(ibu_k_runs_scan, dim3(rows), dim3(kSortThreads), 0, st, seg_heads, nseg, seg_base, totals);
}

size_t runs_scratch_bytes(size_t n) { return runs_layout(n).runs_bytes; }
size_t runs_emit_scratch_bytes(uint64_t n_runs) { return 16 * (size_t)(n_runs ? n_runs : 1); }

hipError_t launch_runs_count(const LaunchCfg& cfg, const void* recs, size_t n, void* scratch, size_t scratch_bytes, RunsCount what, hipStream_t st) {
  (void)hipGetLastError();
  const RunsLayout L = runs_layout(n);
  if (n == 0 || n / kSegRecs + 2 >= (1ull << 31) || scratch_bytes < L.runs_bytes) return hipErrorInvalidValue;
  const SegPlan sp = seg_plan(cfg, recs, n);
  u32* heads = scratch_at<u32>(scratch, L.seg_heads);
  if (what == RunsCount::Pair)
    hipLaunchKernelGGL(ibu_k_pairs_count, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, heads);
  else if (what == RunsCount::BarcodeStash)
    hipLaunchKernelGGL(ibu_k_runs_count_stash, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, heads,
                       scratch_at<RunStash>(scratch, L.stash));
  else
    hipLaunchKernelGGL(ibu_k_runs_count, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, heads);
  launch_runs_scan(heads, sp.nseg, 2, scratch_at<u64>(scratch, L.seg_base), scratch_at<u64>(scratch, L.totals), st);
  return hipGetLastError();
}
hipError_t launch_runs_emit(const LaunchCfg& cfg, const void* recs, size_t n, const void* scratch, void* run_scratch, uint64_t n_runs,
                            uint64_t n_ranked, uint64_t* first, uint64_t* second, uint64_t* counts, uint64_t* distinct, hipStream_t st) {
  (void)hipGetLastError();
  const RunsLayout L = runs_layout(n);
  const SegPlan sp = seg_plan(cfg, recs, n);
  const u64* base = scratch_at<const u64>(scratch, L.seg_base);
  u64* starts = static_cast<u64*>(run_scratch);             // n_runs entries each (runs_emit_scratch_bytes)
  u64* rank = distinct ? starts + n_runs : nullptr;
  if (second)
    hipLaunchKernelGGL(ibu_k_pairs_emit, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, base, (u64*)first, (u64*)second, starts,
                       rank);
  else
    hipLaunchKernelGGL(ibu_k_runs_emit, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, base,
                       scratch_at<const u32>(scratch, L.seg_heads), scratch_at<const RunStash>(scratch, L.stash), (u64*)first, starts, rank);
  hipLaunchKernelGGL(ibu_k_runs_finish, dim3(capped_grid(cfg, n_runs, 256)), dim3(256), 0, st, (const u64*)starts, (const u64*)rank, (u64)n_runs,
                     (u64)n, (u64)n_ranked, (u64*)counts, (u64*)distinct);
  return hipGetLastError();
}
// The last step of a launcher (what was launched in front of it keeps its error): words where the first tiled class byte is 4-byte
// aligned, bytes elsewhere.
hipError_t launch_class_fill(const LaunchCfg& cfg, const void* recs, size_t n, const void* scratch, bool ranked, const uint8_t* verdict,
                             uint8_t* d_class, hipStream_t st) {
  const SegPlan sp = seg_plan(cfg, recs, n);
  const RunsLayout L = runs_layout(n);
  const u64* seg_row = scratch_at<const u64>(scratch, L.seg_base) + (ranked ? sp.nseg : 0);
  const u64* masks = scratch_at<const u64>(scratch, L.mol_masks);
  const bool words = ((reinterpret_cast<uintptr_t>(d_class) + sp.head) & 3u) == 0;
  hipLaunchKernelGGL(words ? ibu_k_class_fill<true> : ibu_k_class_fill<false>, seg_grid(sp), dim3(kSortThreads), 0, st, sp, seg_row, masks,
                     verdict, d_class);
  return hipGetLastError();
}

}  // namespace ibu
