// runs_walk.hpp — the segment walk over SORTED records behind k_aggregate.hip, k_molecules.hip, k_cells.hip, k_saturation.hip,
// k_metrics.hip and k_features.hip: the cut of the rows into segments (SegPlan), the count scratch they address (RunsLayout), the walk
// (runs_segment) with the sinks' three hooks (NoSink: step, head, ballots) and the sink that keeps ballots for the class fill
// (BallotSink), the body of every kernel that walks (walk_wave; runs_kernel: its two-counter form).
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
// record (at most one), segments 1 .. S = 8 Ki records each (64 tiles), segment S+1 = the n % 128 rest.  An untiled end (segment 0,
// segment S+1) has fewer than 128 rows, so at most two steps of 64: the two words it has among the kept ballots (BallotSink) fit.
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
  RunsLayout L;
  L.totals = 0;
  L.seg_heads = 64;
  L.seg_base = align_up(L.seg_heads + 2 * sizeof(u32) * cap, 8);
  L.stash = align_up(L.seg_base + 2 * sizeof(u64) * cap, 16);
  L.runs_bytes = L.stash + sizeof(RunStash) * kStashHeads * cap;    // ibu_barcode_counts, ibu_pair_counts
  L.mol_masks = align_up(L.runs_bytes, 16);
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

// What a walk hands to its SINK, in three hooks.  A sink derives from NoSink and replaces what it needs; NoSink itself only counts,
// and whatever feeds a body left empty (the ranks, the row, a word, a ballot) is never computed or loaded.  What a sink carries from
// step to step (a per-run reduction: k_saturation.hip; counters: k_metrics.hip) lives in `mutable` members of the sink.
// A STEP, as every lane sees it: the lane's record `row` (a) and, in a tiled step (pair), record `row + 1` (b), with three levels of
// head flags each — a0 / b0: the record begins a barcode (barcode_head), a1 / b1: a run, a2 / b2: it is a ranked head; a0 implies a1
// implies a2.  va: a is a record; false in a lane past the end of an untiled step, where a is all zero, its flags are false and the
// row lies at or behind the segment's end.  An untiled step has no b: all zero, flags false.
struct WalkStep { u32 lane; u64 row; Rec a; bool va, a0, a1, a2; Rec b; bool b0, b1, b2, pair; };
struct NoSink {
  // Every step, in EVERY lane, whether it holds a head or not.
  __device__ __forceinline__ void step(const WalkStep&) const {}
  // Every ranked head, in the lane that holds it: `run` runs and `ranked` ranked heads begin in front of it (counted from the two
  // bases the walk was given), `row` is its record, w0 / w1 its first two words, run_head: it begins a run as well.
  __device__ __forceinline__ void head(u64 run, u64 ranked, u64 row, u64 w0, u64 w1, bool run_head) const {}
  // Every step, in lane 0, behind the step's heads: the ballots of run heads and of ranked heads (a superset).  Bit L of `even`
  // is the step's record 2L and bit L of `odd` record 2L + 1 in a tiled step (the 128 records of a tile); an untiled step has its
  // 64 records in `even`.  `at` is the word of the kept-ballot array (below) where the step belongs.
  __device__ __forceinline__ void ballots(u64 at, bool tiled, u64 run_even, u64 run_odd, u64 even, u64 odd) const {}
};

// The sinks that keep a walk's ballots for the class fill (k_aggregate.hip) store them here, and the fill finds them here: masks
// (nullable in a sink: nothing kept) = u64[2 ntiles], tile t's (even, odd) at 2t, then u64[2] per untiled end, one word per step
// (SegPlan: at most two).  MolEmit keeps the ranked heads' ballots this way, CellEmit the run heads', MetricsSink the barcode heads'.
__host__ __device__ constexpr u64 tile_ballots_at(u64 tile) { return 2 * tile; }
__host__ __device__ constexpr u64 end_ballots_at(u64 ntiles, u32 which, u32 step) { return 2 * ntiles + 2 * which + step; }
struct BallotSink : NoSink {
  u64* masks;
  __device__ __forceinline__ void keep(u64 at, bool tiled, u64 even, u64 odd) const {
    if (masks) { masks[at] = even; if (tiled) masks[at + 1] = odd; }
  }
};

// One step of a walk, from what every lane brings (WalkStep): hands the step to the sink, ranks the heads in the wave, hands the
// ranked heads over, adds the step to the counts and, in lane 0, hands over the step's ballots, which belong at word `at`.
struct SegCounts { u64 runs, ranked; };
template <class S>
struct RunRanks {
  const S& sink;
  u32 lane;
  u64 p1, p2, lt_mask;
  SegCounts n;
  __device__ __forceinline__ void step(u64 at, u64 row, const Rec& a, bool va, bool a0, bool a1, bool a2, const Rec& b, bool b0, bool b1,
                                       bool b2, bool pair) {
    sink.step(WalkStep{lane, row, a, va, a0, a1, a2, b, b0, b1, b2, pair});
    const u64 run_even = __ballot(a1), run_odd = __ballot(b1), even = __ballot(a2), odd = __ballot(b2);
    const u64 k = p1 + n.runs + (u64)(__popcll(run_even & lt_mask) + __popcll(run_odd & lt_mask));
    const u64 q = p2 + n.ranked + (u64)(__popcll(even & lt_mask) + __popcll(odd & lt_mask));
    if (a2) sink.head(k, q, row, a.w0, a.w1, a1);
    if (b2) sink.head(k + (a1 ? 1 : 0), q + (a2 ? 1 : 0), row + 1, b.w0, b.w1, b1);
    n.runs += (u64)(__popcll(run_even) + __popcll(run_odd));
    n.ranked += (u64)(__popcll(even) + __popcll(odd));
    if (lane == 0) sink.ballots(at, pair, run_even, run_odd, even, odd);
  }
};

// One wave walks one segment; p1 / p2 = the runs / ranked heads that begin in front of it.  Returns the segment's own two counts.
// The 8 Ki segments are TILED like every streaming kernel here: three coalesced dwordx4 loads stage 128 records in the wave's LDS
// slice while the next tile's loads are in flight, lane L owns records 2L and 2L+1 and reads record 2L-1 from the slice (lane 0: the
// last record of the previous tile, kept in registers; the first tile of a segment: one global load).  No barrier, no atomic.
template <int D, class S>
__device__ __forceinline__ SegCounts runs_segment(const u64* __restrict__ recs, const SegPlan& sp, u32 seg, uint8_t* tile, u32 lane, u64 p1,
                                                  u64 p2, const S& sink) {
  RunRanks<S> ranks{sink, lane, p1, p2, (1ull << lane) - 1, {0, 0}};
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
      ranks.step(end_ballots_at(sp.main / kTileRecs, seg == 0 ? 0u : 1u, (u32)((i0 - base) / kWave)), i, cur, valid,
                 valid && barcode_head(prev, cur, i > 0), valid && h1, valid && h2, none, false, false, false, false);
    }
    return ranks.n;
  }
  const u64 begin = sp.head + (u64)(seg - 1) * kSegRecs;    // 16-B aligned row
  const u64 stop = sp.head + sp.main;
  const u32 ntiles = (u32)(((begin + kSegRecs < stop ? begin + kSegRecs : stop) - begin) / kTileRecs);   // >= 1
  const uint8_t* src = reinterpret_cast<const uint8_t*>(recs + 3 * begin) + 16 * lane;
  bool have_prev = begin > 0;
  Rec carry = have_prev ? load_rec<D>(recs + 3 * (begin - 1)) : none;   // the record in front of the tile
  // NOT sweep_tiles (kcommon.hpp), whose note against copied register sets this loop contradicts knowingly: ONE set, copied at the
  // end of an iteration, so that the body (every sink's step, inlined) is emitted once, not twice.  Moving it there is a performance
  // change that wants its own measurement.  The stage is load_tile / land_tile (kcommon.hpp) WRITTEN OUT, as the note on the tuned
  // kernels there allows: through the helpers the same IR comes out with its phis in another order and ibu_k_cells_emit takes 50
  // VGPRs for 48 (profiles/README.md, r23_a).
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
    ranks.step(tile_ballots_at((begin - sp.head) / kTileRecs + t), begin + (u64)t * kTileRecs + 2 * lane, x, true,
               barcode_head(prev, x, lane > 0 || have_prev), xa, xb, y, barcode_head(x, y, true), ya, yb, true);
    carry = load_rec<D>(reinterpret_cast<const u64*>(tile + (kTileRecs - 1) * 24));   // same address in every lane: one broadcast read
    have_prev = true;
    if (!more) break;
    ++t;
    a0 = b0; a1 = b1; a2 = b2;
  }
  return ranks.n;
}

// The body of every kernel that walks: the LDS slab, this wave's segment and its guard, the segment through `sink`, and then, in
// the same wave, done(seg, lane, counts).  seg_base: the scanned table [2][nseg] from which an emit pass takes the two bases (null:
// count from 0).  A wave without a segment runs neither and comes BACK: the guard leaves this function, never the kernel, so what
// every thread must reach behind the walk (a barrier: ibu_k_feature_count) stays reachable.  The counts are HANDED ON, not returned
// beside a had-a-segment flag: the kernel would test the flag again, this target's compiler threads no jumps, and the count kernels
// paid four SGPRs, zeroed counters and VOP3 compares for it (profiles/README.md, r23_a).
template <int D, class S, class Done>
__device__ __forceinline__ void walk_wave(const u64* __restrict__ recs, const SegPlan& sp, const u64* __restrict__ seg_base, const S& sink,
                                          Done done) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kSortWaves * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 seg = wave_segment();
  if (seg >= sp.nseg) return;                               // wave-uniform
  done(seg, lane, runs_segment<D>(recs, sp, seg, lds + wib * kTileBytes, lane, seg_base ? seg_base[seg] : 0,
                                  seg_base ? seg_base[sp.nseg + seg] : 0, sink));
}
// The two-counter form, count and emit: seg_heads is where a count pass leaves the segment's two counts (null: nowhere).
template <int D, class S>
__device__ __forceinline__ void runs_kernel(const u64* __restrict__ recs, const SegPlan& sp, const u64* __restrict__ seg_base /*[2][nseg]*/,
                                            u32* __restrict__ seg_heads /*[2][nseg]*/, const S& sink) {
  walk_wave<D>(recs, sp, seg_base, sink, [&](u32 seg, u32 lane, SegCounts n) {
    if (seg_heads && lane == 0) { seg_heads[seg] = (u32)n.runs; seg_heads[sp.nseg + seg] = (u32)n.ranked; }
  });
}

// Entry k of a table of neighbour differences: col[k + 1] - col[k], with `end` closing the last of the `count` rows.
__device__ __forceinline__ u64 closed_diff(const u64* col, u64 k, u64 count, u64 end) { return (k + 1 == count ? end : col[k + 1]) - col[k]; }

// The scan of per-segment counts (ibu_k_runs_scan, k_aggregate.hip): seg_heads u32[rows][nseg] -> seg_base u64[rows][nseg], the
// exclusive prefix of every row, and totals[rows], the row sums.  One workgroup per row.
void launch_runs_scan(const u32* seg_heads, u32 nseg, u32 rows, u64* seg_base, u64* totals, hipStream_t st);

}  // namespace ibu
