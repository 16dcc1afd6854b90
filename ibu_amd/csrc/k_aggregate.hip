// k_aggregate.hip — per-barcode aggregation of SORTED records: the device form of the reference's BarcodeAnalyzer
// processor (src/parallel.rs:72-98).  Launchers: launch_runs_count / launch_runs_emit (kernels.h); C ABI: ibu_barcode_counts
// (device.cpp).  Split from sort.hip in round 3: nothing here depends on the sort.
#include "kcommon.hpp"
#include "kernels.h"

namespace ibu {

static constexpr int kSortThreads = 256;                      // one wave per segment, four waves per workgroup
static constexpr int kSortWaves = kSortThreads / kWave;

// =====================================================================================================
// Per-barcode aggregation on SORTED records: the device form of the reference's BarcodeAnalyzer
// processor (src/parallel.rs:72-98: HashMap<barcode, count> merged in on_batch_complete).  On sorted
// input a barcode is a run, so the map is a run-length encoding: barcodes[k], counts[k] and — the
// UMI-dedup figure single-cell pipelines want from exactly this layout — unique_umis[k] = number of
// distinct (barcode, umi) pairs in the run.  Output order = ascending barcode (the map's sorted keys).
//
// The rows are cut into SEGMENTS, one per wave, no barrier anywhere: segment 0 = the peeled rows in front of the first
// 16-B aligned record (at most one), segments 1 .. S = 8 Ki records each (64 tiles), segment S+1 = the n % 128 rest.
// The 8 Ki segments are TILED like every streaming kernel here (round 2; the first version read two stride-24 u64 per
// lane and step with nothing in flight): three coalesced dwordx4 loads stage 128 records in the wave's LDS slice while
// the next tile's loads are in flight, lane L owns records 2L and 2L+1 and reads record 2L-1 from the slice (lane 0: the
// last record of the previous tile, kept in registers; the first tile of a segment: one global load).  Run heads are
// ranked with __ballot / popcount.  Pass 1 counts heads per segment, the [2][nseg] table is scanned, pass 2 emits each
// run's barcode, first record and pair rank with plain stores, and a last small kernel turns neighbouring entries into
// counts (no atomics anywhere: the first version used two per run and took 1 s on 0.9e9 runs of length one).
// =====================================================================================================
//
// Round 5: ONE read of the records where runs are long.  The count pass also keeps the first kStashHeads run heads of every segment
// (barcode, row inside the segment, pair rank inside the segment: 16 bytes each, plain stores — there are few) in a stash in the
// scratch; the emit pass serves a segment with that many heads or fewer FROM THE STASH (a few lanes, no record read) and walks only
// the others again.  Whitelist barcodes (1e5 runs in 1e9 records, 0.8 heads per segment): 24 B/record instead of 48; every record
// its own barcode: as before.
// =====================================================================================================
static constexpr int kSegRecs = 8192;
static constexpr u32 kStashHeads = 32;
struct __attribute__((aligned(16))) RunStash { u64 barcode; u32 row_off; u32 pair_local; };

__device__ __forceinline__ u64 shfl_up64(u64 v) {
  u32 lo = __shfl_up((u32)v, 1), hi = __shfl_up((u32)(v >> 32), 1);
  return ((u64)hi << 32) | lo;
}
// The walk has a DEPTH D.  A run is a maximal stretch of records whose first D words agree; its head is its first record (h1), and
// inside it the records whose word D differs from the record before them are ranked (h2 = h1 || word D differs).  D = 1: runs of a
// barcode, ranked (barcode, umi) pairs — ibu_barcode_counts.  D = 2: runs of a (w0, w1) pair, ranked triples — ibu_pair_counts (in
// the three-level reading: a pair head is "w0 differs or w1 differs", a triple head "a pair head or w2 differs").  The D = 1
// instantiations never look at the third word.
//
// heads of one 64-record step of an untiled segment.  Lanes past `end` are neither.
template <int D>
__device__ __forceinline__ void run_heads(const u64* __restrict__ recs, u64 i, u64 end, u32 lane, u64& b, u64& u, bool& h1, bool& h2) {
  const bool valid = i < end;
  b = valid ? recs[3 * i] : 0;
  u = valid ? recs[3 * i + 1] : 0;
  u64 pb = shfl_up64(b), pu = shfl_up64(u);
  if (lane == 0 && valid && i > 0) { pb = recs[3 * (i - 1)]; pu = recs[3 * (i - 1) + 1]; }
  if constexpr (D == 1) {
    h1 = valid && (i == 0 || b != pb);
    h2 = valid && (h1 || u != pu);
  } else {
    const u64 x = valid ? recs[3 * i + 2] : 0;
    u64 px = shfl_up64(x);
    if (lane == 0 && valid && i > 0) px = recs[3 * (i - 1) + 2];
    h1 = valid && (i == 0 || b != pb || u != pu);
    h2 = valid && (h1 || x != px);
  }
}

struct SegPlan { u64 head, main, n; u32 nseg; };            // rows [0, head) | [head, head + main) tiled | rest
static inline u32 runs_nseg(size_t main_rows) { return (u32)((main_rows + kSegRecs - 1) / kSegRecs) + 2; }
__device__ __forceinline__ u64 seg_first_row(const SegPlan& sp, u32 seg) {
  return seg == 0 ? 0 : (seg == sp.nseg - 1 ? sp.head + sp.main : sp.head + (u64)(seg - 1) * kSegRecs);
}

// One wave walks one segment and hands every run head to `emit(k, w0, w1, row, rank)`; returns the number of
// run heads / ranked heads through c1 / c2.  EMIT = 0: counting only (p1, p2 unused).  EMIT = 2 (ibu_classify_molecules, below): the
// RANKED heads are handed over instead — emit.head(rank, row, is a run head too) — and lane 0 hands every step's ballots of ranked
// heads to emit.masks_tile(tile of the tiled rows, even records, odd records) / emit.masks_end(which end, step, records).
template <int EMIT, int D, class F>
__device__ __forceinline__ void runs_segment(const u64* __restrict__ recs, const SegPlan& sp, u32 seg, uint8_t* tile, u32 lane, u64 p1,
                                             u64 p2, u64& c1, u64& c2, F emit) {
  const u64 lt_mask = (1ull << lane) - 1;
  c1 = c2 = 0;
  if (seg == 0 || seg == sp.nseg - 1) {                     // wave-uniform: the untiled ends (< 128 rows each)
    const u64 base = seg == 0 ? 0 : sp.head + sp.main;
    const u64 end = seg == 0 ? sp.head : sp.n;
    for (u64 i0 = base; i0 < end; i0 += kWave) {
      const u64 i = i0 + lane;
      u64 b, u; bool h1, h2;
      run_heads<D>(recs, i, end, lane, b, u, h1, h2);
      const u64 m1 = __ballot(h1), m2 = __ballot(h2);
      if constexpr (EMIT == 1) {
        if (h1) emit(p1 + c1 + (u64)__popcll(m1 & lt_mask), b, u, i, p2 + c2 + (u64)__popcll(m2 & lt_mask));
      } else if constexpr (EMIT == 2) {
        if (h2) emit.head(p2 + c2 + (u64)__popcll(m2 & lt_mask), i, h1);
        if (lane == 0) emit.masks_end(seg == 0 ? 0u : 1u, (u32)((i0 - base) / kWave), m2);
      }
      c1 += (u64)__popcll(m1);
      c2 += (u64)__popcll(m2);
    }
    return;
  }
  const u64 begin = sp.head + (u64)(seg - 1) * kSegRecs;    // 16-B aligned row
  const u64 stop = sp.head + sp.main;
  const u32 ntiles = (u32)(((begin + kSegRecs < stop ? begin + kSegRecs : stop) - begin) / kTileRecs);   // >= 1
  const uint8_t* src = reinterpret_cast<const uint8_t*>(recs + 3 * begin) + 16 * lane;
  u64 cb = 0, cu = 0, cx = 0;                               // the record in front of the tile (its third word at D = 2 only)
  bool have_prev = begin > 0;
  if (have_prev) {
    cb = recs[3 * (begin - 1)]; cu = recs[3 * (begin - 1) + 1];
    if constexpr (D == 2) cx = recs[3 * (begin - 1) + 2];
  }
  u32x4 a0 = ld16(src), a1 = ld16(src + 1024), a2 = ld16(src + 2048);
  for (u32 t = 0;;) {
    const bool more = t + 1 < ntiles;                       // wave-uniform; the prefetch is unconditional (kcommon.hpp)
    const uint8_t* nx = src + (size_t)(more ? t + 1 : t) * kTileBytes;
    const u32x4 b0 = ld16(nx), b1 = ld16(nx + 1024), b2 = ld16(nx + 2048);
    wave_lds_fence();
    *reinterpret_cast<u32x4*>(tile + 16 * lane) = a0;
    *reinterpret_cast<u32x4*>(tile + 1024 + 16 * lane) = a1;
    *reinterpret_cast<u32x4*>(tile + 2048 + 16 * lane) = a2;
    wave_lds_fence();
    const u64* r = reinterpret_cast<const u64*>(tile + (2 * lane) * 24);  // records 2L, 2L+1 (and 2L-1 just below)
    u64 pb = cb, pu = cu;
    if (lane > 0) { pb = r[-3]; pu = r[-2]; }
    const u64 x0 = r[0], x1 = r[1], y0 = r[3], y1 = r[4];
    bool ha1, ha2, hb1, hb2;
    if constexpr (D == 1) {
      ha1 = !(lane > 0 || have_prev) || x0 != pb; ha2 = ha1 || x1 != pu;
      hb1 = y0 != x0; hb2 = hb1 || y1 != x1;
    } else {
      u64 px = cx;
      if (lane > 0) px = r[-1];
      const u64 x2 = r[2], y2 = r[5];
      ha1 = !(lane > 0 || have_prev) || x0 != pb || x1 != pu; ha2 = ha1 || x2 != px;
      hb1 = y0 != x0 || y1 != x1; hb2 = hb1 || y2 != x2;
    }
    const u64 ma1 = __ballot(ha1), mb1 = __ballot(hb1), ma2 = __ballot(ha2), mb2 = __ballot(hb2);
    if constexpr (EMIT == 2) {
      const u64 row = begin + (u64)t * kTileRecs + 2 * lane;
      const u64 q = p2 + c2 + (u64)(__popcll(ma2 & lt_mask) + __popcll(mb2 & lt_mask));
      if (ha2) emit.head(q, row, ha1);
      if (hb2) emit.head(q + (ha2 ? 1 : 0), row + 1, hb1);
      if (lane == 0) emit.masks_tile((begin - sp.head) / kTileRecs + t, ma2, mb2);
    } else if constexpr (EMIT == 1) {
      const u64 row = begin + (u64)t * kTileRecs + 2 * lane;
      const u64 k = p1 + c1 + (u64)(__popcll(ma1 & lt_mask) + __popcll(mb1 & lt_mask));
      const u64 q = p2 + c2 + (u64)(__popcll(ma2 & lt_mask) + __popcll(mb2 & lt_mask));
      if (ha1) emit(k, x0, x1, row, q);
      if (hb1) emit(k + (ha1 ? 1 : 0), y0, y1, row + 1, q + (ha2 ? 1 : 0));
    }
    c1 += (u64)(__popcll(ma1) + __popcll(mb1));
    c2 += (u64)(__popcll(ma2) + __popcll(mb2));
    const u64* last = reinterpret_cast<const u64*>(tile + (kTileRecs - 1) * 24);
    cb = last[0]; cu = last[1];                              // same address in every lane: one broadcast read
    if constexpr (D == 2) cx = last[2];
    have_prev = true;
    if (!more) break;
    ++t;
    a0 = b0; a1 = b1; a2 = b2;
  }
}

extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_runs_count(const u64* __restrict__ recs, SegPlan sp, u32* __restrict__ seg_heads /*[2][nseg]*/) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;                               // wave-uniform
  u64 c1, c2;
  runs_segment<0, 1>(recs, sp, seg, lds + wib * kTileBytes, lane, 0, 0, c1, c2, [](u64, u64, u64, u64, u64) {});
  if (lane == 0) { seg_heads[seg] = (u32)c1; seg_heads[sp.nseg + seg] = (u32)c2; }
}
// ... and keeping the segment's first kStashHeads heads for the emit pass (see the top of the file)
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_runs_count_stash(const u64* __restrict__ recs, SegPlan sp, u32* __restrict__ seg_heads /*[2][nseg]*/, RunStash* __restrict__ stash /*[nseg][kStashHeads]*/) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;                               // wave-uniform
  u64 c1, c2;
  const u64 row0 = seg_first_row(sp, seg);
  RunStash* mine = stash + (size_t)seg * kStashHeads;
  runs_segment<1, 1>(recs, sp, seg, lds + wib * kTileBytes, lane, 0, 0, c1, c2, [=](u64 k, u64 b, u64, u64 row, u64 q) {
    if (k < kStashHeads) { RunStash e; e.barcode = b; e.row_off = (u32)(row - row0); e.pair_local = (u32)q; mine[k] = e; }
  });
  if (lane == 0) { seg_heads[seg] = (u32)c1; seg_heads[sp.nseg + seg] = (u32)c2; }
}

extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_runs_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/,
                const u32* __restrict__ seg_heads /*[2][nseg]*/, const RunStash* __restrict__ stash /*[nseg][kStashHeads] or null*/,
                u64* __restrict__ barcodes, u64* __restrict__ starts, u64* __restrict__ pair_rank) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;
  if (stash) {                                              // wave-uniform: the heads the count pass kept are all of them
    const u32 heads = seg_heads[seg];
    if (heads <= kStashHeads) {
      if (lane < heads) {
        const RunStash e = stash[(size_t)seg * kStashHeads + lane];
        const u64 k = seg_base[seg] + lane;
        barcodes[k] = e.barcode;
        starts[k] = seg_first_row(sp, seg) + e.row_off;
        if (pair_rank) pair_rank[k] = seg_base[sp.nseg + seg] + e.pair_local;
      }
      return;
    }
  }
  u64 c1, c2;
  // seg_base: runs / pairs that start before this segment
  runs_segment<1, 1>(recs, sp, seg, lds + wib * kTileBytes, lane, seg_base[seg], seg_base[sp.nseg + seg], c1, c2,
                        [=](u64 k, u64 b, u64, u64 row, u64 q) {
                          barcodes[k] = b;
                          starts[k] = row;                   // first record of run k
                          if (pair_rank) pair_rank[k] = q;   // (barcode, umi) pairs that start before it
                        });
}
// The same two passes one level deeper (ibu_pair_counts): runs of equal (w0, w1), the records that begin a new (w0, w1, w2) ranked
// inside them.  No stash: entries are typically a sizeable fraction of the records (a count matrix has a few reads per entry), and
// a segment with more than kStashHeads of them is walked again anyway.
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_pairs_count(const u64* __restrict__ recs, SegPlan sp, u32* __restrict__ seg_heads /*[2][nseg]*/) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;                               // wave-uniform
  u64 c1, c2;
  runs_segment<0, 2>(recs, sp, seg, lds + wib * kTileBytes, lane, 0, 0, c1, c2, [](u64, u64, u64, u64, u64) {});
  if (lane == 0) { seg_heads[seg] = (u32)c1; seg_heads[sp.nseg + seg] = (u32)c2; }
}
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_pairs_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/,
                 u64* __restrict__ first, u64* __restrict__ second, u64* __restrict__ starts, u64* __restrict__ triple_rank) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;
  u64 c1, c2;
  runs_segment<1, 2>(recs, sp, seg, lds + wib * kTileBytes, lane, seg_base[seg], seg_base[sp.nseg + seg], c1, c2,
                        [=](u64 k, u64 w0, u64 w1, u64 row, u64 q) {
                          first[k] = w0;
                          second[k] = w1;
                          starts[k] = row;                        // first record of entry k
                          if (triple_rank) triple_rank[k] = q;    // (w0, w1, w2) heads in front of it
                        });
}
// counts[k] = start(k+1) - start(k), unique_umis[k] = pair_rank(k+1) - pair_rank(k); entry n_runs is the sentinel.
extern "C" __global__ void ibu_k_runs_finish(const u64* __restrict__ starts, const u64* __restrict__ pair_rank, u64 n_runs, u64 n,
                                             u64 n_pairs, u64* __restrict__ counts, u64* __restrict__ uniq) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < n_runs; k += stride) {
    const bool last = k + 1 == n_runs;
    counts[k] = (last ? n : starts[k + 1]) - starts[k];
    if (uniq) uniq[k] = (last ? n_pairs : pair_rank[k + 1]) - pair_rank[k];
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

static SegPlan seg_plan(const LaunchCfg& cfg, const void* recs, size_t n) {
  const Span span[1] = {{recs, 24}};
  const RowSplit rs = split_rows(cfg, span, 1, n, kTileRecs);    // an 8-B aligned base peels exactly one record
  return {(u64)rs.head, (u64)rs.main, (u64)n, runs_nseg(rs.main)};
}
static inline size_t seg_base_offset(u32 nseg) { return 64 + 2 * sizeof(u32) * (size_t)nseg + ((2 * sizeof(u32) * (size_t)nseg) & 4); }
static inline size_t stash_offset(u32 nseg) { return (seg_base_offset(nseg) + 2 * sizeof(u64) * (size_t)nseg + 15) & ~(size_t)15; }
size_t runs_scratch_bytes(size_t n) {
  const u32 nseg = runs_nseg(n);                             // main <= n
  return stash_offset(nseg) + sizeof(RunStash) * kStashHeads * (size_t)nseg;   // totals u64[2] | seg_heads u32[2][nseg] | pad | seg_base u64[2][nseg] | pad | stash
}
// Pass 1 + scan.  Leaves the scanned table in `scratch`; totals[0] = runs, totals[1] = (barcode, umi) pairs
// are read back by the caller from scratch[0..15] (u64 each).
// keep_heads: the emit pass follows (launch_runs_emit with from_stash = true); false: a size query.
hipError_t launch_runs_count(const LaunchCfg& cfg, const void* recs, size_t n, void* scratch, size_t scratch_bytes, bool keep_heads, hipStream_t st,
                             bool pair_level) {
  (void)hipGetLastError();
  if (n == 0 || n / kSegRecs + 2 >= (1ull << 31) || scratch_bytes < runs_scratch_bytes(n)) return hipErrorInvalidValue;
  const SegPlan sp = seg_plan(cfg, recs, n);
  u64* totals = static_cast<u64*>(scratch);
  u32* heads = reinterpret_cast<u32*>(static_cast<uint8_t*>(scratch) + 64);
  u64* base = reinterpret_cast<u64*>(static_cast<uint8_t*>(scratch) + seg_base_offset(sp.nseg));
  if (pair_level)
    hipLaunchKernelGGL(ibu_k_pairs_count, dim3((sp.nseg + kSortWaves - 1) / kSortWaves), dim3(kSortThreads), 0, st, (const u64*)recs, sp,
                       heads);
  else if (keep_heads)
    hipLaunchKernelGGL(ibu_k_runs_count_stash, dim3((sp.nseg + kSortWaves - 1) / kSortWaves), dim3(kSortThreads), 0, st, (const u64*)recs, sp,
                       heads, reinterpret_cast<RunStash*>(static_cast<uint8_t*>(scratch) + stash_offset(sp.nseg)));
  else
    hipLaunchKernelGGL(ibu_k_runs_count, dim3((sp.nseg + kSortWaves - 1) / kSortWaves), dim3(kSortThreads), 0, st, (const u64*)recs, sp,
                       heads);
  hipLaunchKernelGGL(ibu_k_runs_scan, dim3(2), dim3(kSortThreads), 0, st, (const u32*)heads, sp.nseg, base, totals);
  return hipGetLastError();
}
hipError_t launch_runs_emit(const LaunchCfg& cfg, const void* recs, size_t n, const void* scratch, bool from_stash, void* run_scratch, uint64_t n_runs,
                            uint64_t n_pairs, uint64_t* barcodes, uint64_t* counts, uint64_t* uniq, hipStream_t st) {
  (void)hipGetLastError();
  const SegPlan sp = seg_plan(cfg, recs, n);
  const u32* heads = reinterpret_cast<const u32*>(static_cast<const uint8_t*>(scratch) + 64);
  const u64* base = reinterpret_cast<const u64*>(static_cast<const uint8_t*>(scratch) + seg_base_offset(sp.nseg));
  const RunStash* stash = from_stash ? reinterpret_cast<const RunStash*>(static_cast<const uint8_t*>(scratch) + stash_offset(sp.nseg)) : nullptr;
  u64* starts = static_cast<u64*>(run_scratch);             // n_runs entries each (run_scratch_bytes)
  u64* pair_rank = uniq ? starts + n_runs : nullptr;
  hipLaunchKernelGGL(ibu_k_runs_emit, dim3((sp.nseg + kSortWaves - 1) / kSortWaves), dim3(kSortThreads), 0, st, (const u64*)recs, sp,
                     base, heads, stash, (u64*)barcodes, starts, pair_rank);
  u64 blocks = (n_runs + 255) / 256;
  const u64 cap = (u64)cfg.cus * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(ibu_k_runs_finish, dim3((u32)(blocks ? blocks : 1)), dim3(256), 0, st, (const u64*)starts, (const u64*)pair_rank,
                     (u64)n_runs, (u64)n, (u64)n_pairs, (u64*)counts, (u64*)uniq);
  return hipGetLastError();
}
hipError_t launch_pairs_emit(const LaunchCfg& cfg, const void* recs, size_t n, const void* scratch, void* run_scratch, uint64_t n_pairs,
                             uint64_t n_triples, uint64_t* first, uint64_t* second, uint64_t* counts, uint64_t* distinct, hipStream_t st) {
  (void)hipGetLastError();
  const SegPlan sp = seg_plan(cfg, recs, n);
  const u64* base = reinterpret_cast<const u64*>(static_cast<const uint8_t*>(scratch) + seg_base_offset(sp.nseg));
  u64* starts = static_cast<u64*>(run_scratch);             // n_pairs entries each (runs_emit_scratch_bytes)
  u64* triple_rank = distinct ? starts + n_pairs : nullptr;
  hipLaunchKernelGGL(ibu_k_pairs_emit, dim3((sp.nseg + kSortWaves - 1) / kSortWaves), dim3(kSortThreads), 0, st, (const u64*)recs, sp,
                     base, (u64*)first, (u64*)second, starts, triple_rank);
  u64 blocks = (n_pairs + 255) / 256;
  const u64 cap = (u64)cfg.cus * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(ibu_k_runs_finish, dim3((u32)(blocks ? blocks : 1)), dim3(256), 0, st, (const u64*)starts, (const u64*)triple_rank,
                     (u64)n_pairs, (u64)n, (u64)n_triples, (u64*)counts, (u64*)distinct);
  return hipGetLastError();
}
size_t runs_emit_scratch_bytes(uint64_t n_runs) { return 16 * (size_t)(n_runs ? n_runs : 1); }

// =====================================================================================================
// ibu_classify_molecules: one index per (barcode, umi) molecule.  A molecule is a run of equal (w0, w1), a candidate a run of equal
// (w0, w1, w2) inside it; the candidate with strictly the most records is kept (class 0), the others are minor (1), and a molecule
// whose top is shared is tied (2) — include/ibu_hip.h has the rule in full.  Five steps, the records read twice:
//   count    ibu_k_pairs_count + ibu_k_runs_scan as for ibu_pair_counts: molecules and candidates per segment, scanned; the two
//            totals go back to the host to size the candidate table.
//   emit     the D = 2 walk again, handing over the TRIPLE heads: table[c] = first row of candidate c, bit 63 set where it begins a
//            molecule (8 bytes per candidate), and, when class bytes are wanted, the walk's own ballots of triple heads (16 bytes
//            per 128-record tile) — the fill pass needs nothing else of the records.
//   verdict  one workgroup per 1024 candidates: reads(c) = start(c + 1) - start(c), a segmented scan of (best, how many at best, first
//            at best) over the block, every molecule's total dropped in LDS under its ordinal in the block and picked up by its
//            candidates.  Molecules inside a block are settled here (one verdict byte per candidate, the totals per wave, per block,
//            one atomic per block and total).  The piece in front of a block's first molecule head and the piece behind its last one
//            are left to the two kernels below together with their partial aggregates.
//   chains   one workgroup runs the same segmented scan over the blocks' summaries, 1024 per round: a molecule that leaves its
//            block gets its total at the block it began in.  fix: every block settles its two open pieces from those totals.  A
//            molecule of any length costs a constant per candidate this way: 1e6 candidates are 977 blocks, one round here.
//   fill     one wave per segment turns the ballots into each record's candidate number (popcounts, no record read, no LDS) and
//            writes the verdicts as class bytes, four records per lane and store.
// =====================================================================================================
static constexpr u64 kMolHead = 1ull << 63;
static constexpr u64 kRowMask = (1ull << 40) - 1;
static constexpr u32 kMolItems = 4;
static constexpr u32 kMolBlock = kSortThreads * kMolItems;    // candidates per verdict workgroup
static constexpr u32 kNoChain = 0xFFFFFFFFu;

// best reads << 4 | min(2, candidates at best) << 2 | min(2, candidates); first = the first candidate at best; s = the block a chain
// began in (ibu_k_molecules_chains only).  key == 0: nothing.
struct MolAgg { u64 key; u64 first; u32 s; };
__device__ __forceinline__ MolAgg mol_none() { return {0, 0, kNoChain}; }
__device__ __forceinline__ MolAgg mol_combine(const MolAgg a, const MolAgg b) {   // a in front of b
  const u64 ak = a.key, bk = b.key, af = a.first, bf = b.first;   // (values, not references: a select between two fields must not become one between two addresses)
  const u32 as = a.s, bs = b.s;
  const u64 ba = ak >> 4, bb = bk >> 4;
  const u32 ca = (u32)(ak >> 2) & 3u, cb = (u32)(bk >> 2) & 3u;
  u32 nn = ((u32)ak & 3u) + ((u32)bk & 3u);
  nn = nn < 2 ? nn : 2;
  u32 cc = ca + cb;
  cc = cc < 2 ? cc : 2;
  const bool a_wins = ba > bb, b_wins = bb > ba;
  MolAgg r;
  r.s = bs != kNoChain ? bs : as;
  r.key = ((a_wins ? ba : bb) << 4) | ((a_wins ? ca : b_wins ? cb : cc) << 2) | nn;
  r.first = (a_wins || (!b_wins && ca)) ? af : bf;
  return r;
}
__device__ __forceinline__ u64 shfl_up64d(u64 v, int d) {
  const u32 lo = __shfl_up((u32)v, d), hi = __shfl_up((u32)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}
struct MolScanLds { MolAgg v[kSortWaves]; u32 f[kSortWaves]; };
// Segmented scan over the 256 threads of a workgroup.  Thread t brings (f, v): f = one of its items begins a segment, v = the aggregate
// of its items behind its last segment start (all of them when f is false).  Returns what is open in front of the thread — the
// aggregate from the last segment start before it, `carry` included where no thread in front has one — and leaves in *total what is
// open behind the last thread.
__device__ __forceinline__ MolAgg mol_block_scan(bool f, MolAgg v, const MolAgg& carry, MolScanLds* lds, MolAgg* total) {
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  u32 ff = f ? 1u : 0u;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    MolAgg p;
    p.key = shfl_up64d(v.key, d); p.first = shfl_up64d(v.first, d); p.s = __shfl_up(v.s, d);
    const u32 pf = __shfl_up(ff, d);
    if (lane >= (u32)d) {
      if (!ff) v = mol_combine(p, v);
      ff |= pf;
    }
  }
  if (lane == kWave - 1) { lds->v[wib] = v; lds->f[wib] = ff; }
  __syncthreads();
  MolAgg in = carry, all = carry;                          // open in front of this wave / behind the last one
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) {
    const MolAgg wv = lds->v[w];
    all = lds->f[w] ? wv : mol_combine(all, wv);
    if ((u32)w + 1 == wib) in = all;
  }
  __syncthreads();                                          // the slots may be reused by the caller's next scan
  *total = all;
  const MolAgg inc = ff ? v : mol_combine(in, v);
  MolAgg ex;
  ex.key = shfl_up64d(inc.key, 1); ex.first = shfl_up64d(inc.first, 1); ex.s = __shfl_up(inc.s, 1);
  return lane == 0 ? in : ex;
}
__device__ __forceinline__ u32 mol_class(const MolAgg& m, u64 c, u32 tie_first) {
  if (((m.key >> 2) & 3u) >= 2 && !tie_first) return 2;     // IBU_MOLECULE_TIED
  return c == m.first ? 0u : 1u;                            // KEPT : MINOR
}
// one candidate into a thread's five totals (static indices only: the array stays in registers)
__device__ __forceinline__ void mol_tally(u64 (&t)[5], u32 cls, u64 reads, bool mol_head, u64 key) {
  t[2] += cls == 0 ? reads : 0;
  t[3] += cls == 1 ? reads : 0;
  t[4] += cls == 2 ? reads : 0;
  const bool several = mol_head && (key & 3u) >= 2, top_shared = ((key >> 2) & 3u) >= 2;
  t[0] += several && !top_shared ? 1 : 0;
  t[1] += several && top_shared ? 1 : 0;
}
// acc: [0] resolved molecules, [1] tied molecules, [2..4] records of class 0, 1, 2
__device__ __forceinline__ void mol_accumulate(u64 (&t)[5], u64* acc, u64* lds /*[kSortWaves][5]*/) {
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const u32 lo = __shfl_xor((u32)t[k], m), hi = __shfl_xor((u32)(t[k] >> 32), m);
      t[k] += ((u64)hi << 32) | lo;
    }
    if (lane == 0) lds[wib * 5 + k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) s += lds[w * 5 + threadIdx.x];
    if (s) atomicAdd(&acc[threadIdx.x], s);
  }
}

struct MolEmit {
  u64* table; u64* masks; u64 ntiles;
  __device__ __forceinline__ void head(u64 c, u64 row, bool mol_head) const { table[c] = row | (mol_head ? kMolHead : 0); }
  __device__ __forceinline__ void masks_tile(u64 tile, u64 even, u64 odd) const {
    if (masks) { masks[2 * tile] = even; masks[2 * tile + 1] = odd; }
  }
  __device__ __forceinline__ void masks_end(u32 which, u32 step, u64 m) const {
    if (masks && step < 2) masks[2 * ntiles + 2 * which + step] = m;
  }
};
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_molecules_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/, u64* __restrict__ table,
                     u64* __restrict__ masks /*nullable*/) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;
  u64 c1, c2;
  const MolEmit e{table, masks, sp.main / kTileRecs};
  runs_segment<2, 2>(recs, sp, seg, lds + wib * kTileBytes, lane, seg_base[seg], seg_base[sp.nseg + seg], c1, c2, e);
}

// What a verdict block leaves for the chain scan: the aggregate of the candidates in front of its first molecule head (`lead`, all
// of the block when it has none) and of those from its last molecule head on when that molecule goes on in the next block (`trail`).
struct __attribute__((aligned(16))) MolSummary { u64 lead_key, lead_first, trail_key, trail_first; u32 lead_len, trail_off, has_head, open; };
struct __attribute__((aligned(16))) MolFull { u64 key, first; };

extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_verdict(const u64* __restrict__ table, u64 ncand, u64 n, u32 tie_first, uint8_t* __restrict__ verdict, MolSummary* __restrict__ summary,
                        u64* __restrict__ acc) {
  __shared__ MolFull tot[kMolBlock + 1];                    // slot 0: the lead piece; slot m: the block's m-th molecule
  __shared__ MolScanLds scan;
  __shared__ u32 wsum[kSortWaves];
  __shared__ u64 accl[kSortWaves * 5];
  __shared__ u32 s_lead_len, s_trail_off, s_open;
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x * kMolBlock, c0 = base + kMolItems * tid;
  const u32 in_block = (u32)(ncand - base < kMolBlock ? ncand - base : kMolBlock);
  if (tid == 0) { s_lead_len = in_block; s_trail_off = 0; s_open = 0; }
  const u64 sentinel = n | kMolHead;
  u64 e[kMolItems + 1];
#pragma unroll
  for (u32 j = 0; j <= kMolItems; ++j) e[j] = c0 + j < ncand ? table[c0 + j] : sentinel;
  MolAgg run = mol_none();
  bool seen = false;
  u32 nh = 0;
#pragma unroll
  for (u32 j = 0; j < kMolItems; ++j) {
    const bool valid = c0 + j < ncand;
    const u64 reads = (e[j + 1] & kRowMask) - (e[j] & kRowMask);
    const MolAgg item = valid ? MolAgg{(reads << 4) | 5u, c0 + j, kNoChain} : mol_none();
    if (e[j] & kMolHead) { run = item; seen = true; nh += valid ? 1u : 0u; }
    else run = mol_combine(run, item);
  }
  MolAgg unused;
  run = mol_block_scan(seen, run, mol_none(), &scan, &unused);   // now: what is open in front of this thread's candidates
  u32 nheads;
  u32 m = block_exclusive_scan(nh, wsum, &nheads);           // molecule heads of the block in front of this thread
  u32 slot[kMolItems];
#pragma unroll
  for (u32 j = 0; j < kMolItems; ++j) {
    const bool valid = c0 + j < ncand;
    const u64 reads = (e[j + 1] & kRowMask) - (e[j] & kRowMask);
    const MolAgg item = valid ? MolAgg{(reads << 4) | 5u, c0 + j, kNoChain} : mol_none();
    const bool head = valid && (e[j] & kMolHead);
    run = (e[j] & kMolHead) ? item : mol_combine(run, item);  // the molecule from its beginning in the block to this candidate
    if (head) {
      ++m;
      if (m == 1) s_lead_len = kMolItems * tid + j;
      if (m == nheads) s_trail_off = kMolItems * tid + j;
    }
    const bool block_end = kMolItems * tid + j + 1 == kMolBlock;
    if (valid && ((e[j + 1] & kMolHead) || block_end)) {
      tot[m] = MolFull{run.key, run.first};
      if (block_end && !(e[j + 1] & kMolHead)) s_open = 1;
    }
    slot[j] = m;
  }
  __syncthreads();
  const u32 open = nheads ? s_open : 0;                     // (a block without a molecule head is all lead)
  u64 t[5] = {0, 0, 0, 0, 0};
  u32 packed = 0;
#pragma unroll
  for (u32 j = 0; j < kMolItems; ++j) {
    const bool settled = c0 + j < ncand && slot[j] >= 1 && !(open && slot[j] == nheads);
    if (settled) {
      const MolFull f = tot[slot[j]];
      const MolAgg mol{f.key, f.first, 0};
      const u32 cls = mol_class(mol, c0 + j, tie_first);
      const u64 reads = (e[j + 1] & kRowMask) - (e[j] & kRowMask);
      packed |= cls << (8 * j);
      mol_tally(t, cls, reads, (e[j] & kMolHead) != 0, f.key);
    }
  }
  if (c0 < ncand) *reinterpret_cast<u32*>(verdict + c0) = packed;   // (the array is padded to a multiple of four; open pieces: ibu_k_molecules_fix)
  if (tid == 0) {
    MolSummary sm;
    const bool has_lead = s_lead_len > 0;
    sm.lead_key = has_lead ? tot[0].key : 0; sm.lead_first = has_lead ? tot[0].first : 0;
    sm.trail_key = open ? tot[nheads].key : 0; sm.trail_first = open ? tot[nheads].first : 0;
    sm.lead_len = s_lead_len; sm.trail_off = s_trail_off; sm.has_head = nheads ? 1u : 0u; sm.open = open;
    summary[blockIdx.x] = sm;
  }
  mol_accumulate(t, acc, accl);
}

// One workgroup.  Block j enters the scan as a segment start with its trail when it has a molecule head, and as its lead (all of
// it) otherwise; what is open in front of j, joined with j's lead, is the total of the molecule that ends in j.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_chains(const MolSummary* __restrict__ summary, u32 nblk, u32* __restrict__ chain_start, MolFull* __restrict__ chain_full) {
  __shared__ MolScanLds scan;
  MolAgg carry = mol_none();
  for (u32 base = 0; base < nblk; base += kMolBlock) {      // (block-uniform trip count: the scan has barriers)
    const u32 j0 = base + kMolItems * threadIdx.x;
    MolAgg run = mol_none();
    bool seen = false;
#pragma unroll
    for (u32 k = 0; k < kMolItems; ++k) {
      if (j0 + k < nblk) {
        const MolSummary sm = summary[j0 + k];
        if (sm.has_head) { run = MolAgg{sm.trail_key, sm.trail_first, j0 + k}; seen = true; }
        else run = mol_combine(run, MolAgg{sm.lead_key, sm.lead_first, kNoChain});
      }
    }
    MolAgg total;
    run = mol_block_scan(seen, run, carry, &scan, &total);    // now: what is open in front of this thread's blocks
    carry = total;
#pragma unroll
    for (u32 k = 0; k < kMolItems; ++k) {
      const u32 j = j0 + k;
      if (j < nblk) {
        const MolSummary sm = summary[j];
        const MolAgg lead{sm.lead_key, sm.lead_first, kNoChain};
        if (sm.lead_len && run.s != kNoChain) {
          chain_start[j] = run.s;
          if (sm.has_head || j + 1 == nblk) { const MolAgg f = mol_combine(run, lead); chain_full[run.s] = MolFull{f.key, f.first}; }
        }
        run = sm.has_head ? MolAgg{sm.trail_key, sm.trail_first, j} : mol_combine(run, lead);
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_fix(const u64* __restrict__ table, u64 ncand, u64 n, u32 tie_first, const MolSummary* __restrict__ summary,
                    const u32* __restrict__ chain_start, const MolFull* __restrict__ chain_full, uint8_t* __restrict__ verdict, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves * 5];
  const MolSummary sm = summary[blockIdx.x];
  if (!sm.lead_len && !sm.open) return;                     // block-uniform: every molecule of the block was settled in it
  const u64 base = (u64)blockIdx.x * kMolBlock;
  const u32 in_block = (u32)(ncand - base < kMolBlock ? ncand - base : kMolBlock);
  u64 t[5] = {0, 0, 0, 0, 0};
  for (int piece = 0; piece < 2; ++piece) {
    if (piece == 0 ? !sm.lead_len : !sm.open) continue;
    u32 from = piece == 0 ? chain_start[blockIdx.x] : blockIdx.x;
    from = from < gridDim.x ? from : 0;                      // (never taken: a lead piece has a block with a molecule head in front of it)
    const MolFull f = chain_full[from];
    const MolAgg mol{f.key, f.first, 0};
    const u32 lo = piece == 0 ? 0 : sm.trail_off, hi = piece == 0 ? sm.lead_len : in_block;
    for (u32 i = lo + threadIdx.x; i < hi; i += kSortThreads) {
      const u64 c = base + i;
      const u64 next = c + 1 < ncand ? table[c + 1] & kRowMask : n;
      const u32 cls = mol_class(mol, c, tie_first);
      verdict[c] = (uint8_t)cls;
      mol_tally(t, cls, next - (table[c] & kRowMask), piece == 1 && i == lo /*the molecule head is here*/, f.key);
    }
  }
  mol_accumulate(t, acc, accl);
}

// Class bytes from the ballots the emit pass kept.  One wave per segment, as in the walk; in a tiled segment lane L first takes tile
// L's two ballots and the wave ranks the tiles, then every step serves two tiles: lanes 0-31 the first, lanes 32-63 the second, four
// consecutive records (two even, two odd positions of the walk's lane pairs) per lane.
template <bool WORDS>
__global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_fill(SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/, const u64* __restrict__ masks,
                     const uint8_t* __restrict__ verdict, uint8_t* __restrict__ d_class) {
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = blockIdx.x * kSortWaves + wib;
  if (seg >= sp.nseg) return;                               // wave-uniform
  const u64 cbase = seg_base[sp.nseg + seg];                // candidates that begin in front of the segment
  const u64 ntiles_all = sp.main / kTileRecs;
  if (seg == 0 || seg == sp.nseg - 1) {
    const u64 begin = seg == 0 ? 0 : sp.head + sp.main, end = seg == 0 ? sp.head : sp.n;
    u64 seen = 0;
    for (u32 step = 0; step < 2; ++step) {
      const u64 i = begin + (u64)step * kWave + lane;
      if (begin + (u64)step * kWave >= end) break;           // wave-uniform
      const u64 m = masks[2 * ntiles_all + 2 * (seg == 0 ? 0 : 1) + step];
      if (i < end) d_class[i] = verdict[cbase + seen + (u64)__popcll(m & ((2ull << lane) - 1)) - 1];
      seen += (u64)__popcll(m);
    }
    return;
  }
  const u64 begin = sp.head + (u64)(seg - 1) * kSegRecs, stop = sp.head + sp.main;
  const u32 ntiles = (u32)(((begin + kSegRecs < stop ? begin + kSegRecs : stop) - begin) / kTileRecs);   // 1 .. 64
  const u64 tile0 = (begin - sp.head) / kTileRecs;
  u64 even = 0, odd = 0;
  if (lane < ntiles) { even = masks[2 * (tile0 + lane)]; odd = masks[2 * (tile0 + lane) + 1]; }
  const u32 mine = (u32)(__popcll(even) + __popcll(odd));
  u32 rank = mine;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const u32 up = __shfl_up(rank, d);
    if (lane >= (u32)d) rank += up;
  }
  rank -= mine;                                             // candidates that begin in the segment's tiles in front of tile `lane`
  const u32 l = lane & 31u;
  const u64 below = (1ull << (2 * l)) - 1;
  for (u32 step = 0; 2 * step < ntiles; ++step) {
    const u32 tile = 2 * step + (lane >> 5);
    const u64 ev = ((u64)__shfl((u32)(even >> 32), tile) << 32) | __shfl((u32)even, tile);
    const u64 od = ((u64)__shfl((u32)(odd >> 32), tile) << 32) | __shfl((u32)odd, tile);
    const u32 r0 = __shfl(rank, tile);
    if (tile < ntiles) {
      // records 4l .. 4l+3 of the tile = the walk's (lane 2l: even, odd), (lane 2l+1: even, odd)
      const u64 k0 = cbase + r0 + (u64)(__popcll(ev & below) + __popcll(od & below)) + ((ev >> (2 * l)) & 1) - 1;
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

// run scratch: acc u64[8] | table u64[ncand] | verdict bytes | summaries | chain starts | chain totals
struct MolLayout { size_t table, verdict, summary, chain_start, chain_full, bytes; u32 nblk; };
static MolLayout mol_layout(uint64_t ncand) {
  MolLayout L;
  L.nblk = (u32)((ncand + kMolBlock - 1) / kMolBlock);
  const size_t nb = L.nblk ? L.nblk : 1;
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  L.table = 64;
  L.verdict = up(L.table + 8 * (size_t)(ncand ? ncand : 1));
  L.summary = up(L.verdict + (size_t)ncand + 4);
  L.chain_start = up(L.summary + sizeof(MolSummary) * nb);
  L.chain_full = up(L.chain_start + sizeof(u32) * nb);
  L.bytes = up(L.chain_full + sizeof(MolFull) * nb);
  return L;
}
size_t molecules_run_scratch_bytes(uint64_t candidates) { return mol_layout(candidates).bytes; }
static inline size_t mol_masks_offset(size_t n) { return (runs_scratch_bytes(n) + 15) & ~(size_t)15; }
size_t molecules_scratch_bytes(size_t n) { return mol_masks_offset(n) + sizeof(u64) * (2 * (n / kTileRecs) + 4); }
hipError_t launch_molecules_classify(const LaunchCfg& cfg, const void* recs, size_t n, void* scratch, void* run_scratch, uint64_t candidates,
                                     bool tie_first, uint8_t* d_class, hipStream_t st) {
  (void)hipGetLastError();
  if (candidates == 0 || candidates > n || n >= (1ull << 40)) return hipErrorInvalidValue;
  const SegPlan sp = seg_plan(cfg, recs, n);
  const u64* base = reinterpret_cast<const u64*>(static_cast<const uint8_t*>(scratch) + seg_base_offset(sp.nseg));
  u64* masks = d_class ? reinterpret_cast<u64*>(static_cast<uint8_t*>(scratch) + mol_masks_offset(n)) : nullptr;
  const MolLayout L = mol_layout(candidates);
  uint8_t* rs = static_cast<uint8_t*>(run_scratch);
  u64* acc = reinterpret_cast<u64*>(rs);
  u64* table = reinterpret_cast<u64*>(rs + L.table);
  uint8_t* verdict = rs + L.verdict;
  MolSummary* summary = reinterpret_cast<MolSummary*>(rs + L.summary);
  u32* chain_start = reinterpret_cast<u32*>(rs + L.chain_start);
  MolFull* chain_full = reinterpret_cast<MolFull*>(rs + L.chain_full);
  hipError_t e = hipMemsetAsync(acc, 0, 64, st);
  if (e != hipSuccess) return e;
  const dim3 seg_grid((sp.nseg + kSortWaves - 1) / kSortWaves);
  hipLaunchKernelGGL(ibu_k_molecules_emit, seg_grid, dim3(kSortThreads), 0, st, (const u64*)recs, sp, base, table, masks);
  hipLaunchKernelGGL(ibu_k_molecules_verdict, dim3(L.nblk), dim3(kSortThreads), 0, st, (const u64*)table, (u64)candidates, (u64)n,
                     tie_first ? 1u : 0u, verdict, summary, acc);
  hipLaunchKernelGGL(ibu_k_molecules_chains, dim3(1), dim3(kSortThreads), 0, st, (const MolSummary*)summary, L.nblk, chain_start, chain_full);
  hipLaunchKernelGGL(ibu_k_molecules_fix, dim3(L.nblk), dim3(kSortThreads), 0, st, (const u64*)table, (u64)candidates, (u64)n,
                     tie_first ? 1u : 0u, (const MolSummary*)summary, (const u32*)chain_start, (const MolFull*)chain_full, verdict, acc);
  if (d_class) {
    if (((reinterpret_cast<uintptr_t>(d_class) + sp.head) & 3u) == 0)
      hipLaunchKernelGGL(ibu_k_molecules_fill<true>, seg_grid, dim3(kSortThreads), 0, st, sp, base, (const u64*)masks, (const uint8_t*)verdict, d_class);
    else
      hipLaunchKernelGGL(ibu_k_molecules_fill<false>, seg_grid, dim3(kSortThreads), 0, st, sp, base, (const u64*)masks, (const uint8_t*)verdict, d_class);
  }
  return hipGetLastError();
}

}  // namespace ibu
