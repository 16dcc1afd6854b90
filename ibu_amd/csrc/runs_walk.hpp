// runs_walk.hpp — the segment walk over SORTED records that k_aggregate.hip (barcode and pair counts) and k_molecules.hip (one index
// per molecule) share: the cut of the rows into segments (SegPlan), the count scratch both address (RunsLayout), the walk itself
// (runs_segment) with the sinks' interface (NoSink) and the sink that keeps the ballots for the class fill (BallotSink), the body of
// every kernel that runs it (runs_kernel).  k_cells.hip (cell calling) and k_saturation.hip (the saturation curve: a per-run minimum carried from tile to tile through NoSink::records) walk it too, and
// k_metrics.hip (per-barcode QC metrics: three levels of heads and a set test, through NoSink::words).
#pragma once
#include "kcommon.hpp"
#include "kernels.h"

namespace ibu {

static constexpr int kSortThreads = 256;                      // one wave per segment, four waves per workgroup
static constexpr int kSortWaves = kSortThreads / kWave;
static_assert(kSortThreads == kBlock, "the kernels of the walk sum their totals with block_accumulate (kcommon.hpp): a workgroup of kBlock");
static constexpr int kSegRecs = 8192;
static constexpr u32 kStashHeads = 32;
struct __attribute__((aligned(16))) RunStash { u64 barcode; u32 row_off; u32 pair_local; };

// The rows are cut into SEGMENTS, one per wave, no barrier anywhere: segment 0 = the peeled rows in front of the first 16-B aligned
// record (at most one), segments 1 .. S = 8 Ki records each (64 tiles), segment S+1 = the n % 128 rest.
struct SegPlan { u64 head, main, n; u32 nseg; };            // rows [0, head) | [head, head + main) tiled | rest
static inline u32 runs_nseg(size_t main_rows) { return (u32)((main_rows + kSegRecs - 1) / kSegRecs) + 2; }
static inline SegPlan seg_plan(const LaunchCfg& cfg, const void* recs, size_t n) {
  const Span span[1] = {{recs, 24}};
  const RowSplit rs = split_rows(cfg, span, 1, n, kTileRecs);    // an 8-B aligned base peels exactly one record
  return {(u64)rs.head, (u64)rs.main, (u64)n, runs_nseg(rs.main)};
}
__device__ __forceinline__ u64 seg_first_row(const SegPlan& sp, u32 seg) {
  return seg == 0 ? 0 : (seg == sp.nseg - 1 ? sp.head + sp.main : sp.head + (u64)(seg - 1) * kSegRecs);
}
__device__ __forceinline__ u32 wave_segment() { return blockIdx.x * kSortWaves + (threadIdx.x >> 6); }
static inline dim3 seg_grid(const SegPlan& sp) { return dim3((sp.nseg + kSortWaves - 1) / kSortWaves); }

// The count scratch (byte offsets): totals u64[2] | seg_heads u32[2][cap] | seg_base u64[2][cap], scanned | stash [cap][kStashHeads]
// | the ballots the class fill turns into class bytes, u64[2 (n / 128) + 4]: (even, odd) of every tile, then two steps of each
// untiled end (BallotSink below; ranked heads: ibu_classify_molecules; run heads: ibu_call_cells; one region, one call at a time).
// It is a function of n alone, so that a scratch sized before the records' base is known fits them at any alignment: cap = runs_nseg(n) segments, while a plan has sp.nseg = runs_nseg(sp.main) <= cap of them (one
// fewer where peeling a record moves the last tile into the rest).  The tables are PLACED by cap and INDEXED with sp.nseg as their row
// length, [row * sp.nseg + seg], which stays inside them.
struct RunsLayout { size_t totals, seg_heads, seg_base, stash, runs_bytes, mol_masks, mol_bytes; };
static inline RunsLayout runs_layout(size_t n) {
  const size_t cap = runs_nseg(n);
  auto up = [](size_t x, size_t a) { return (x + a - 1) & ~(a - 1); };
  RunsLayout L;
  L.totals = 0;
  L.seg_heads = 64;
  L.seg_base = up(L.seg_heads + 2 * sizeof(u32) * cap, 8);
  L.stash = up(L.seg_base + 2 * sizeof(u64) * cap, 16);
  L.runs_bytes = L.stash + sizeof(RunStash) * kStashHeads * cap;    // ibu_barcode_counts, ibu_pair_counts
  L.mol_masks = up(L.runs_bytes, 16);
  L.mol_bytes = L.mol_masks + sizeof(u64) * (2 * (n / kTileRecs) + 4);   // ibu_classify_molecules, ibu_call_cells
  return L;
}
template <class T> static inline T* scratch_at(const void* scratch, size_t off) {
  return reinterpret_cast<T*>(static_cast<uint8_t*>(const_cast<void*>(scratch)) + off);
}

// The walk has a DEPTH D.  A run is a maximal stretch of records whose first D words agree; its head is its first record (h1), and
// inside it the records whose word D differs from the record before them are ranked (h2 = h1 || word D differs).  D = 1: runs of a
// barcode, ranked (barcode, umi) pairs — ibu_barcode_counts.  D = 2: runs of a (w0, w1) pair, ranked triples — ibu_pair_counts,
// ibu_classify_molecules.  The D = 1 instantiations never load the third word.
struct Rec { u64 w0, w1, w2; };
template <int D>
__device__ __forceinline__ Rec load_rec(const u64* p) { return {p[0], p[1], D == 2 ? p[2] : 0}; }
template <int D>
__device__ __forceinline__ void run_head(const Rec& prev, const Rec& cur, bool has_prev, bool& h1, bool& h2) {
  h1 = !has_prev || cur.w0 != prev.w0 || (D == 2 && cur.w1 != prev.w1);
  h2 = h1 || (D == 1 ? cur.w1 != prev.w1 : cur.w2 != prev.w2);
}
// The level above the runs of a D = 2 walk: the record begins a BARCODE, its w0 differs from the record before it (D = 1: a run head).
__device__ __forceinline__ bool barcode_head(const Rec& prev, const Rec& cur, bool has_prev) { return !has_prev || cur.w0 != prev.w0; }

// What a walk hands to its SINK.  A sink derives from NoSink and replaces what it needs; NoSink itself only counts, and whatever
// feeds a body left empty (the ranks, the row) is never computed.
struct NoSink {
  // Every ranked head, in the lane that holds it: `run` runs and `ranked` ranked heads begin in front of it (counted from the two
  // bases the walk was given), `row` is its record, w0 / w1 its first two words, run_head: it begins a run as well.
  __device__ __forceinline__ void head(u64 run, u64 ranked, u64 row, u64 w0, u64 w1, bool run_head) const {}
  // Every step, in lane 0, the ballots of ranked heads.  A tiled step covers tile `tile` of the main rows: bit L of `even` is record
  // 2L of the tile, bit L of `odd` record 2L + 1.  A step of an untiled end (which = 0: the rows in front, 1: the rest) covers its
  // records 64 step .. 64 step + 63.
  __device__ __forceinline__ void tile_ballots(u64 tile, u64 even, u64 odd) const {}
  __device__ __forceinline__ void end_ballots(u32 which, u32 step, u64 m) const {}
  // The same steps, the ballots of RUN heads (a subset of the ranked heads), laid out alike.
  __device__ __forceinline__ void tile_run_ballots(u64 tile, u64 even, u64 odd) const {}
  __device__ __forceinline__ void end_run_ballots(u32 which, u32 step, u64 m) const {}
  // Every step, in EVERY lane, whether it holds a head or not: the lane's record `row` (a) with its run-head flag a1 and its
  // ranked-head flag a2, and, in a tiled step (pair), record `row + 1` (b) with b1 / b2.  A lane past the end of an untiled step
  // comes with a row at or behind the segment's end and both flags false.  What a sink carries from step to step (a per-run
  // reduction: k_saturation.hip) lives in `mutable` members of the sink.
  __device__ __forceinline__ void records(u64 row, bool a1, bool a2, bool b1, bool b2, bool pair) const {}
  // The same steps, in every lane, with the records' WORDS and a third level of heads (k_metrics.hip): a / b as in `records`, va: a
  // is a record (false in a lane past the end of an untiled step, where a is all zero), a0 / b0: the record begins a barcode — its
  // w0 differs from the record before it — and a1, a2, b1, b2 the flags `records` gets.  a0 implies a1 implies a2.
  __device__ __forceinline__ void words(u64 row, const Rec& a, bool va, bool a0, bool a1, bool a2, const Rec& b, bool b0, bool b1, bool b2,
                                        bool pair) const {}
};

// The sinks that keep a walk's ballots for the class fill (k_aggregate.hip) store them here, and the fill finds them here: masks
// (nullable in a sink: nothing kept) = u64[2 ntiles], tile t's (even, odd) at 2t, then u64[2] per untiled end, its first two steps
// (an end has fewer than 128 rows).  MolEmit keeps the ranked heads' ballots this way, CellEmit the run heads'.
__host__ __device__ constexpr u64 tile_ballots_at(u64 tile) { return 2 * tile; }
__host__ __device__ constexpr u64 end_ballots_at(u64 ntiles, u32 which, u32 step) { return 2 * ntiles + 2 * which + step; }
struct BallotSink : NoSink {
  u64* masks; u64 ntiles;
  __device__ __forceinline__ void keep_tile(u64 tile, u64 even, u64 odd) const {
    if (masks) { masks[tile_ballots_at(tile)] = even; masks[tile_ballots_at(tile) + 1] = odd; }
  }
  __device__ __forceinline__ void keep_end(u32 which, u32 step, u64 m) const {
    if (masks && step < 2) masks[end_ballots_at(ntiles, which, step)] = m;
  }
};

// One step of a walk: every lane brings record `row` (a) and, in a tiled step, `row + 1` (b) with their head flags.  Ranks them in
// the wave, hands the ranked heads to the sink and adds the step to the counts; leaves the two ballots of ranked heads (even, odd)
// and the two of run heads (run_even, run_odd).
template <class S>
struct RunRanks {
  const S& sink;
  u64 p1, p2, lt_mask, c1, c2, even, odd, run_even, run_odd;
  __device__ __forceinline__ void step(u64 row, const Rec& a, bool va, bool a0, bool a1, bool a2, const Rec& b, bool b0, bool b1, bool b2,
                                       bool pair) {
    sink.records(row, a1, a2, b1, b2, pair);
    sink.words(row, a, va, a0, a1, a2, b, b0, b1, b2, pair);
    const u64 ma1 = __ballot(a1), mb1 = __ballot(b1);
    run_even = ma1; run_odd = mb1;
    even = __ballot(a2); odd = __ballot(b2);
    const u64 k = p1 + c1 + (u64)(__popcll(ma1 & lt_mask) + __popcll(mb1 & lt_mask));
    const u64 q = p2 + c2 + (u64)(__popcll(even & lt_mask) + __popcll(odd & lt_mask));
    if (a2) sink.head(k, q, row, a.w0, a.w1, a1);
    if (b2) sink.head(k + (a1 ? 1 : 0), q + (a2 ? 1 : 0), row + 1, b.w0, b.w1, b1);
    c1 += (u64)(__popcll(ma1) + __popcll(mb1));
    c2 += (u64)(__popcll(even) + __popcll(odd));
  }
};

// One wave walks one segment; p1 / p2 = the runs / ranked heads that begin in front of it.  Returns the segment's own two counts
// through c1 / c2.  The 8 Ki segments are TILED like every streaming kernel here: three coalesced dwordx4 loads stage 128 records in
// the wave's LDS slice while the next tile's loads are in flight, lane L owns records 2L and 2L+1 and reads record 2L-1 from the slice
// (lane 0: the last record of the previous tile, kept in registers; the first tile of a segment: one global load).  No barrier and no
// atomic anywhere.
template <int D, class S>
__device__ __forceinline__ void runs_segment(const u64* __restrict__ recs, const SegPlan& sp, u32 seg, uint8_t* tile, u32 lane, u64 p1,
                                             u64 p2, u64& c1, u64& c2, const S& sink) {
  RunRanks<S> ranks{sink, p1, p2, (1ull << lane) - 1, 0, 0, 0, 0, 0, 0};
  const Rec none{0, 0, 0};
  if (seg == 0 || seg == sp.nseg - 1) {                     // wave-uniform: the untiled ends (< 128 rows each)
    const u64 base = seg == 0 ? 0 : sp.head + sp.main;
    const u64 end = seg == 0 ? sp.head : sp.n;
    for (u64 i0 = base; i0 < end; i0 += kWave) {
      const u64 i = i0 + lane;
      const bool valid = i < end;                           // lanes past the end hold no head
      const Rec cur = valid ? load_rec<D>(recs + 3 * i) : none;
      Rec prev{shfl_up64(cur.w0, 1), shfl_up64(cur.w1, 1), D == 2 ? shfl_up64(cur.w2, 1) : 0};
      if (lane == 0 && valid && i > 0) prev = load_rec<D>(recs + 3 * (i - 1));
      bool h1, h2;
      run_head<D>(prev, cur, i > 0, h1, h2);
      ranks.step(i, cur, valid, valid && barcode_head(prev, cur, i > 0), valid && h1, valid && h2, none, false, false, false, false);
      if (lane == 0) {
        sink.end_ballots(seg == 0 ? 0u : 1u, (u32)((i0 - base) / kWave), ranks.even);
        sink.end_run_ballots(seg == 0 ? 0u : 1u, (u32)((i0 - base) / kWave), ranks.run_even);
      }
    }
    c1 = ranks.c1; c2 = ranks.c2;
    return;
  }
  const u64 begin = sp.head + (u64)(seg - 1) * kSegRecs;    // 16-B aligned row
  const u64 stop = sp.head + sp.main;
  const u32 ntiles = (u32)(((begin + kSegRecs < stop ? begin + kSegRecs : stop) - begin) / kTileRecs);   // >= 1
  const uint8_t* src = reinterpret_cast<const uint8_t*>(recs + 3 * begin) + 16 * lane;
  bool have_prev = begin > 0;
  Rec carry = have_prev ? load_rec<D>(recs + 3 * (begin - 1)) : none;   // the record in front of the tile
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
    Rec prev = carry;
    if (lane > 0) prev = load_rec<D>(r - 3);
    const Rec x = load_rec<D>(r), y = load_rec<D>(r + 3);
    bool xa, xb, ya, yb;
    run_head<D>(prev, x, lane > 0 || have_prev, xa, xb);
    run_head<D>(x, y, true, ya, yb);
    ranks.step(begin + (u64)t * kTileRecs + 2 * lane, x, true, barcode_head(prev, x, lane > 0 || have_prev), xa, xb, y, barcode_head(x, y, true), ya,
               yb, true);
    if (lane == 0) {
      sink.tile_ballots((begin - sp.head) / kTileRecs + t, ranks.even, ranks.odd);
      sink.tile_run_ballots((begin - sp.head) / kTileRecs + t, ranks.run_even, ranks.run_odd);
    }
    carry = load_rec<D>(reinterpret_cast<const u64*>(tile + (kTileRecs - 1) * 24));   // same address in every lane: one broadcast read
    have_prev = true;
    if (!more) break;
    ++t;
    a0 = b0; a1 = b1; a2 = b2;
  }
  c1 = ranks.c1; c2 = ranks.c2;
}

// The body of every kernel that walks: this wave's segment through `sink`.  seg_base: the scanned table, from which an emit pass
// takes the two bases (null: count from 0).  seg_heads: where a count pass leaves the segment's two counts (null: nowhere).
template <int D, class S>
__device__ __forceinline__ void runs_kernel(const u64* __restrict__ recs, const SegPlan& sp, const u64* __restrict__ seg_base /*[2][nseg]*/,
                                            u32* __restrict__ seg_heads /*[2][nseg]*/, const S& sink) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = wave_segment();
  if (seg >= sp.nseg) return;                               // wave-uniform
  u64 c1, c2;
  runs_segment<D>(recs, sp, seg, lds + wib * kTileBytes, lane, seg_base ? seg_base[seg] : 0, seg_base ? seg_base[sp.nseg + seg] : 0, c1, c2,
                  sink);
  if (seg_heads && lane == 0) { seg_heads[seg] = (u32)c1; seg_heads[sp.nseg + seg] = (u32)c2; }
}

// The scan of per-segment counts (ibu_k_runs_scan, k_aggregate.hip): seg_heads u32[rows][nseg] -> seg_base u64[rows][nseg], the
// exclusive prefix of every row, and totals[rows], the row sums.  One workgroup per row.
void launch_runs_scan(const u32* seg_heads, u32 nseg, u32 rows, u64* seg_base, u64* totals, hipStream_t st);

}  // namespace ibu
