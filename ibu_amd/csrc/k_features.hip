// k_features.hip — ibu_feature_metrics and ibu_filter_features: the other axis of the count matrix.  Per FEATURE (the value f of a
// record's word feature_word, 1 or 2) its reads, its UMIs (triples) and the cells (pairs) it was seen in, and the filter that drops
// the features seen in too few cells — include/ibu_hip.h has the rules in full.  Three kernels:
//   count    the D = 2 walk of runs_walk.hpp with FeatureSink on NoSink::step.  Inside a step the records of a GROUP are adjacent
//            (feature_word 1: a pair; 2: a triple; and whatever the step's first record continues), so the lane that holds a group's
//            first record takes the group's extent and its triple heads from the step's head ballots — kcommon.hpp, next_head,
//            as ibu_k_abundance_add merges the runs of a tile — and issues at most three 8-byte integer atomics into the
//            columns: reads += records, umis += triple heads, cells += 1 where the group begins with a real pair head.  The adds commute: nothing is carried from step to
//            step, and the sums are integers, so two runs give the same columns.  The columns are 8 B per feature and live in L2.
//            Records with f >= n_features enter no column; they and the in-range sums go to per-lane totals and block_accumulate.
//   verdict  a grid-stride loop over the features: the verdict byte from the three columns and the limits, features per class
//            through block_accumulate.
//   class    a per-record pass (kcommon.hpp: sweep_records, store_class_pair, launch_record_pass): one gathered verdict byte per
//            record (the table is n_features bytes and cache resident), reads per class per wave and workgroup.
// No LDS beyond the tiles and block_accumulate's, no scratch memory.  Launchers: launch_feature_count, launch_feature_filter
// (kernels.h); C ABI: api_analysis.cpp.
#include "runs_walk.hpp"

namespace ibu {

__device__ __forceinline__ u64 lanes_below(u32 k) { return k >= 64u ? ~0ull : (1ull << k) - 1; }
__device__ __forceinline__ void feat_add(u64* __restrict__ col, u64 f, u64 v) {   // no value comes back: a no-return atomic
  (void)__hip_atomic_fetch_add(col + f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct FeatureCols { u64* reads; u64* umis; u64* cells; u64 nf; u32 word; };   // each column nullable; word: 1 or 2

// The positions of a step: record `a` of lane L at 2L, record `b` at 2L + 1; an untiled step has no `b`, so its records sit at the
// even positions alone and a distance of positions is twice a distance of records.
struct FeatureSink : NoSink {
  FeatureCols c;
  mutable u64 t_reads, t_umis, t_cells, t_out;                // per lane: in-range reads, umis, cells; reads out of range
  // the group of feature f over positions [pos, next): te / to = the step's ballots of triple heads at even / odd positions
  __device__ __forceinline__ void group(u64 f, u32 pos, u32 next, bool pair, bool pair_head, u64 te, u64 to) const {
    const u64 records = pair ? next - pos : (next - pos) >> 1;
    const bool in = f < c.nf;
    const u64 evens = te & lanes_below((next + 1) >> 1) & ~lanes_below((pos + 1) >> 1);   // 2L in [pos, next)
    const u64 odds = to & lanes_below(next >> 1) & ~lanes_below(pos >> 1);                // 2L + 1 in [pos, next)
    const u64 heads = (u64)(__popcll(evens) + __popcll(odds));
    const bool cell = c.word == 1 && pair_head;
    if (in) {
      if (c.reads) feat_add(c.reads, f, records);
      if (c.umis && heads) feat_add(c.umis, f, heads);
      if (c.cells && cell) feat_add(c.cells, f, 1);
    }
    // every total is added to whatever `in` says: with an add to ONE of t_reads / t_out the compiler picks the total by address,
    // and the four of them live in scratch memory
    t_reads += in ? records : 0; t_umis += in ? heads : 0; t_cells += in && cell ? 1 : 0; t_out += in ? 0 : records;
  }
  __device__ __forceinline__ void step(const WalkStep& s) const {
    const u32 lane = s.lane;
    const bool ga = s.va && (lane == 0 || (c.word == 1 ? s.a1 : s.a2));   // (wave-uniform choice) the step's first record begins a group too
    const bool gb = s.pair && (c.word == 1 ? s.b1 : s.b2);
    const u64 ge = __ballot(ga), go = __ballot(gb), te = __ballot(s.a2), to = __ballot(s.b2);
    const u32 end = 2u * (u32)__popcll(__ballot(s.va));       // the valid lanes are the first ones
    const u32 next = next_head(ge, go, lane, end);            // the first group head behind this lane's records, or the step's end
    if (ga) group(c.word == 1 ? s.a.w1 : s.a.w2, 2 * lane, gb ? 2 * lane + 1 : next, s.pair, s.a1, te, to);
    if (gb) group(c.word == 1 ? s.b.w1 : s.b.w2, 2 * lane + 1, next, s.pair, s.b1, te, to);
  }
};

// acc (nullable, uniform over the grid; block_accumulate): [0] reads in range, [1] umis in range, [2] cells in range, [3] reads out of range
extern "C" __global__ void __launch_bounds__(kSortThreads, 4)
ibu_k_feature_count(const u64* __restrict__ recs, SegPlan sp, FeatureCols cols, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves * 4];
  const FeatureSink sink{{}, cols, 0, 0, 0, 0};
  walk_wave<2>(recs, sp, nullptr, sink, [](u32, u32, SegCounts) {});   // (a wave without a segment comes back too: the barrier below)
  u64 t[4] = {sink.t_reads, sink.t_umis, sink.t_cells, sink.t_out};
  if (acc) block_accumulate(t, acc, accl);
}

// a NULL column counts as 0 everywhere (the entry point refuses a NULL column whose limits are not both 0)
// acc (block_accumulate): [0 .. 2] features per verdict
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_feature_verdict(const u64* __restrict__ reads, const u64* __restrict__ umis, const u64* __restrict__ cells, u64 nf, FeatureLimits lim,
                      uint8_t* __restrict__ verdict, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves * 3];
  u64 t[3] = {0, 0, 0};
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 f = (u64)blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride) {
    const u64 r = reads ? reads[f] : 0, u = umis ? umis[f] : 0, c = cells ? cells[f] : 0;
    const bool low = r < lim.min_reads || u < lim.min_umis || c < lim.min_cells;
    const bool high = (lim.max_reads && r > lim.max_reads) || (lim.max_umis && u > lim.max_umis) || (lim.max_cells && c > lim.max_cells);
    const u32 v = low ? 1u : high ? 2u : 0u;
    verdict[f] = (uint8_t)v;
#pragma unroll
    for (u32 k = 0; k < 3; ++k) t[k] += v == k ? 1 : 0;
  }
  block_accumulate(t, acc, accl);
}

__device__ __forceinline__ u32 feature_class(const uint8_t* __restrict__ verdict, u64 nf, u64 f) { return f < nf ? (u32)verdict[f] : 3u; }

// acc (nullable, uniform over the grid; block_accumulate): [0 .. 3] records per class
struct FeatureClassArgs { const uint8_t* verdict; u64 nf; u32 word; u64* acc; };

extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_feature_class(const uint8_t* __restrict__ recs, u32 ntiles, uint8_t* __restrict__ cls_out /*nullable*/, const FeatureClassArgs fa) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kTileBytes];
  __shared__ u64 accl[kWavesPerBlock * 4];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  uint8_t* tile = lds + wib * kTileBytes;
  u64 t[4] = {0, 0, 0, 0};
  sweep_records(recs, ntiles, tile, lane, wib, [&](u32 k) {
    u32 c[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      c[h] = feature_class(fa.verdict, fa.nf, rec_word(tile, lane, h, fa.word));
#pragma unroll
      for (u32 q = 0; q < 4; ++q) t[q] += c[h] == q ? 1 : 0;
    }
    if (cls_out) store_class_pair(cls_out, k, lane, c[0], c[1]);   // wave-uniform
  });
  if (fa.acc) block_accumulate(t, fa.acc, accl);
}

// One thread per record: the rows peeled off the front of an 8- but not 16-byte aligned array and the n % 128 rest.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_feature_class_tail(const u64* __restrict__ recs, u64 row0, u64 row1, uint8_t* __restrict__ cls_out /*nullable*/, const FeatureClassArgs fa) {
  __shared__ u64 accl[kWavesPerBlock * 4];
  const u64 i = row0 + (u64)blockIdx.x * kBlock + threadIdx.x;
  u64 t[4] = {0, 0, 0, 0};
  if (i < row1) {
    const u32 c = feature_class(fa.verdict, fa.nf, recs[3 * i + fa.word]);
    if (cls_out) cls_out[i] = (uint8_t)c;
#pragma unroll
    for (u32 q = 0; q < 4; ++q) t[q] = c == q ? 1 : 0;
  }
  if (fa.acc) block_accumulate(t, fa.acc, accl);
}

bool feature_args_ok(uint32_t feature_word, uint64_t n_features) {
  return (feature_word == 1 || feature_word == 2) && n_features >= 1 && n_features <= (1ull << 32);
}
// run scratch: acc u64[16] | verdict bytes (when the caller keeps no table of its own)
size_t feature_run_scratch_bytes(uint64_t verdict_bytes) { return align_up(kFeatureAccBytes + verdict_bytes, 16); }

hipError_t launch_feature_count(const LaunchCfg& cfg, const void* recs, size_t n, uint32_t feature_word, uint64_t n_features, uint64_t* d_reads,
                                uint64_t* d_umis, uint64_t* d_cells, uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  if (n >= (1ull << 40) || !feature_args_ok(feature_word, n_features) || (feature_word == 2 && d_cells)) return hipErrorInvalidValue;
  const hipError_t e = zero_totals(acc, 4, st);
  if (e != hipSuccess || n == 0) return e;
  const SegPlan sp = seg_plan(cfg, recs, n);
  hipLaunchKernelGGL(ibu_k_feature_count, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp,
                     FeatureCols{(u64*)d_reads, (u64*)d_umis, (u64*)d_cells, (u64)n_features, feature_word}, (u64*)acc);
  return hipGetLastError();
}

hipError_t launch_feature_filter(const LaunchCfg& cfg, const void* recs, size_t n, uint32_t feature_word, uint64_t n_features,
                                 const uint64_t* d_reads, const uint64_t* d_umis, const uint64_t* d_cells, const FeatureLimits& limits,
                                 uint8_t* verdict, uint8_t* d_class, bool class_totals, uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  if (n >= (1ull << 40) || !feature_args_ok(feature_word, n_features) || !verdict) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(acc, 0, kFeatureAccBytes, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ibu_k_feature_verdict, dim3(capped_grid(cfg, n_features, kSortThreads)), dim3(kSortThreads), 0, st, (const u64*)d_reads,
                     (const u64*)d_umis, (const u64*)d_cells, (u64)n_features, limits, verdict, (u64*)acc);
  if (n == 0 || (!d_class && !class_totals)) return hipGetLastError();
  u64* racc = class_totals ? (u64*)acc + 4 : nullptr;
  launch_record_pass<ibu_k_feature_class, ibu_k_feature_class_tail>(cfg, recs, n, d_class,
                                                                    FeatureClassArgs{verdict, (u64)n_features, feature_word, racc}, st);
  return hipGetLastError();
}

}  // namespace ibu
