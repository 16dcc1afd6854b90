// k_metrics.hip — ibu_barcode_metrics and ibu_filter_barcodes: the per-barcode QC table (reads, pairs, triples, and the reads and
// triples whose word `set_word` lies in a feature set) and the filter made from it.  A barcode is a run of equal w0, a pair a run of
// equal (w0, w1), a triple a run of equal (w0, w1, w2); the set is a bitmap — include/ibu_hip.h has the rules in full.  The records
// are read twice and nothing goes to the host between the steps but the barcode total:
//   count    the D = 2 walk of runs_walk.hpp (its run heads are pair heads, its ranked heads triple heads) with MetricsSink on
//            NoSink::step, which brings the records' words and the barcode-head flag: five counters per segment — barcode
//            heads, pair heads, triple heads, records in the set, triple heads in the set — carried in the sink from step to step
//            as k_saturation.hip carries its state.  ibu_k_runs_scan of k_aggregate.hip turns the five rows into bases and totals; the totals go
//            back to the host to size the table.
//   emit     the walk again: at every barcode head its w0 and the five PREFIX values (its row, and the pair heads, triple heads,
//            set records and set triple heads that lie in front of it), from ballots and popcounts under lt_mask as RunRanks ranks
//            its heads; 40 B per barcode (+ 8 for the barcode column).  For the filter the barcode heads' ballots are kept where
//            launch_class_fill(ranked = false) finds them, beside the barcode heads' bases.
//   table    metric[k] = prefix[k + 1] - prefix[k], the totals closing the last row (ibu_barcode_metrics), or
//   verdict  one class byte per barcode from the same differences and the limits, the totals through block_accumulate
//            (ibu_filter_barcodes), then launch_class_fill of k_aggregate.hip.
// The set test is a gather of one 64-bit word per record from the bitmap (60 000 features: 7.5 KB, resident in L2 and mostly in the
// vector L1); a NULL set costs no load.  No atomic per record or per barcode, no LDS beyond the walk's tiles.
// Launchers: launch_metrics_count, launch_metrics_table, launch_metrics_filter (kernels.h); C ABI: api_analysis.cpp.
#include "runs_walk.hpp"

namespace ibu {

struct FeatureSet {
  const u64* bits; u64 nbits; u32 word;                       // word: 1 or 2, the record word that is looked up
  __device__ __forceinline__ bool has(const Rec& r) const {
    const u64 v = word == 1 ? r.w1 : r.w2;                    // (wave-uniform choice)
    return v < nbits && ((bits[v >> 6] >> (v & 63)) & 1) != 0;
  }
};

// The five counters: [0] barcode heads, [1] pair heads, [2] triple heads, [3] records in the set, [4] triple heads in the set.
// EMIT = false: n[] counts the segment from 0.  EMIT = true: n[] starts at the segment's bases, and every barcode head leaves its
// prefix row: prefix[c * nb + k], c = 0 the row itself, c = 1 .. 4 the counters [1] .. [4] in front of it.
template <bool EMIT>
struct MetricsSink : BallotSink {
  FeatureSet set;
  u64 lt_mask;                                                // (a member, not made from WalkStep::lane in the step: 78 VGPRs for 76 that way)
  u64* barcode /*nullable*/; u64* prefix; u64 nb;
  mutable u64 n0, n1, n2, n3, n4;                             // wave-uniform, carried from step to step
  mutable u64 bar_even, bar_odd;                              // the step's ballots of barcode heads
  __device__ __forceinline__ void put(u64 k, u64 w0, u64 row, u64 r1, u64 r2, u64 r3, u64 r4) const {
    if (barcode) barcode[k] = w0;
    prefix[k] = row;
    prefix[nb + k] = r1;
    prefix[2 * nb + k] = r2;
    prefix[3 * nb + k] = r3;
    prefix[4 * nb + k] = r4;
  }
  __device__ __forceinline__ void step(const WalkStep& s) const {
    const Rec &a = s.a, &b = s.b;
    const bool a0 = s.a0, a1 = s.a1, a2 = s.a2, b0 = s.b0, b1 = s.b1, b2 = s.b2;
    const bool a3 = s.va && set.has(a), b3 = s.pair && set.has(b);
    const bool a4 = a3 && a2, b4 = b3 && b2;
    const u64 m0a = __ballot(a0), m0b = __ballot(b0), m1a = __ballot(a1), m1b = __ballot(b1), m2a = __ballot(a2), m2b = __ballot(b2);
    const u64 m3a = __ballot(a3), m3b = __ballot(b3), m4a = __ballot(a4), m4b = __ballot(b4);
    if constexpr (EMIT) {
      bar_even = m0a; bar_odd = m0b;
      if (a0 || b0) {                                         // few lanes: a barcode is many records
        const u64 k = n0 + (u64)(__popcll(m0a & lt_mask) + __popcll(m0b & lt_mask));
        const u64 r1 = n1 + (u64)(__popcll(m1a & lt_mask) + __popcll(m1b & lt_mask));
        const u64 r2 = n2 + (u64)(__popcll(m2a & lt_mask) + __popcll(m2b & lt_mask));
        const u64 r3 = n3 + (u64)(__popcll(m3a & lt_mask) + __popcll(m3b & lt_mask));
        const u64 r4 = n4 + (u64)(__popcll(m4a & lt_mask) + __popcll(m4b & lt_mask));
        if (a0) put(k, a.w0, s.row, r1, r2, r3, r4);
        if (b0) put(k + (a0 ? 1 : 0), b.w0, s.row + 1, r1 + (a1 ? 1 : 0), r2 + (a2 ? 1 : 0), r3 + (a3 ? 1 : 0), r4 + (a4 ? 1 : 0));
      }
    }
    n0 += (u64)(__popcll(m0a) + __popcll(m0b));
    n1 += (u64)(__popcll(m1a) + __popcll(m1b));
    n2 += (u64)(__popcll(m2a) + __popcll(m2b));
    n3 += (u64)(__popcll(m3a) + __popcll(m3b));
    n4 += (u64)(__popcll(m4a) + __popcll(m4b));
  }
  // the class fill wants the ballots of BARCODE heads, which the walk does not take: kept from `step` of the same step
  __device__ __forceinline__ void ballots(u64 at, bool tiled, u64, u64, u64, u64) const { if constexpr (EMIT) keep(at, tiled, bar_even, bar_odd); }
};

static constexpr u32 kMetricRows = 5;

// seg_heads: u32[5][nseg], the segment's five counters
extern "C" __global__ void __launch_bounds__(kSortThreads, 4)
ibu_k_metrics_count(const u64* __restrict__ recs, SegPlan sp, FeatureSet set, u32* __restrict__ seg_heads) {
  const MetricsSink<false> sink{{{}, nullptr}, set, 0, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0};
  walk_wave<2>(recs, sp, nullptr, sink, [&](u32 seg, u32 lane, SegCounts) {
    if (lane != 0) return;
    seg_heads[seg] = (u32)sink.n0;
    seg_heads[sp.nseg + seg] = (u32)sink.n1;
    seg_heads[2 * sp.nseg + seg] = (u32)sink.n2;
    seg_heads[3 * sp.nseg + seg] = (u32)sink.n3;
    seg_heads[4 * sp.nseg + seg] = (u32)sink.n4;
  });
}

extern "C" __global__ void __launch_bounds__(kSortThreads, 4)
ibu_k_metrics_emit(const u64* __restrict__ recs, SegPlan sp, FeatureSet set, const u64* __restrict__ base0, const u64* __restrict__ base14,
                   u64* __restrict__ barcode /*nullable*/, u64* __restrict__ prefix /*[5][nb]*/, u64 nb, u64* __restrict__ masks /*nullable*/) {
  const u32 seg = wave_segment();
  if (seg >= sp.nseg) return;                                 // wave-uniform: the five bases are read here, in front of the walk
  const MetricsSink<true> sink{{{}, masks}, set, (1ull << (threadIdx.x & (kWave - 1))) - 1, barcode, prefix, nb, base0[seg], base14[seg],
                               base14[sp.nseg + seg], base14[2 * sp.nseg + seg], base14[3 * sp.nseg + seg], 0, 0};
  walk_wave<2>(recs, sp, nullptr, sink, [](u32, u32, SegCounts) {});
}

// column c of barcode k: prefix[c][k + 1] - prefix[c][k]; the row behind the last barcode is (n, totals[1 .. 4])
__device__ __forceinline__ u64 metric_at(const u64* __restrict__ prefix, u64 nb, u64 n, const u64* __restrict__ totals, u32 c, u64 k) {
  return closed_diff(prefix + (size_t)c * nb, k, nb, c == 0 ? n : totals[c]);
}
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_metrics_table(const u64* __restrict__ prefix, u64 nb, u64 n, const u64* __restrict__ totals, u64* __restrict__ reads, u64* __restrict__ pairs,
                    u64* __restrict__ triples, u64* __restrict__ set_reads, u64* __restrict__ set_triples) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < nb; k += stride) {
    if (reads) reads[k] = metric_at(prefix, nb, n, totals, 0, k);
    if (pairs) pairs[k] = metric_at(prefix, nb, n, totals, 1, k);
    if (triples) triples[k] = metric_at(prefix, nb, n, totals, 2, k);
    if (set_reads) set_reads[k] = metric_at(prefix, nb, n, totals, 3, k);
    if (set_triples) set_triples[k] = metric_at(prefix, nb, n, totals, 4, k);
  }
}

// acc (block_accumulate): [0 .. 3] barcodes per class, [4 .. 7] reads per class, [8] triples of class 0, [9] set triples of class 0
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_metrics_verdict(const u64* __restrict__ prefix, u64 nb, u64 n, const u64* __restrict__ totals, MetricsLimits lim,
                      uint8_t* __restrict__ verdict /*nullable*/, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves * 10];
  u64 t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < nb; k += stride) {
    const u64 reads = metric_at(prefix, nb, n, totals, 0, k), pairs = metric_at(prefix, nb, n, totals, 1, k);
    const u64 triples = metric_at(prefix, nb, n, totals, 2, k);
    const u64 set_reads = metric_at(prefix, nb, n, totals, 3, k), set_triples = metric_at(prefix, nb, n, totals, 4, k);
    const bool low = reads < lim.min_reads || pairs < lim.min_pairs || triples < lim.min_triples;
    const bool high = (lim.max_reads && reads > lim.max_reads) || (lim.max_pairs && pairs > lim.max_pairs) ||
                      (lim.max_triples && triples > lim.max_triples);
    // counts below 2^40, set_num <= set_den < 2^24: no product overflows
    const bool over = lim.set_den && (lim.set_of ? set_triples : set_reads) * lim.set_den > lim.set_num * (lim.set_of ? triples : reads);
    const u32 cls = low ? 1u : high ? 2u : over ? 3u : 0u;
    if (verdict) verdict[k] = (uint8_t)cls;
#pragma unroll
    for (u32 c = 0; c < 4; ++c) {
      t[c] += cls == c ? 1 : 0;
      t[4 + c] += cls == c ? reads : 0;
    }
    t[8] += cls == 0 ? triples : 0;
    t[9] += cls == 0 ? set_triples : 0;
  }
  block_accumulate(t, acc, accl);
}

// count scratch (inside runs_layout(n), whose seg_base row 0 and ballots the class fill reads): the five counters per segment and
// the bases of rows 1 .. 4 lie where the barcode-level aggregation keeps its stash — 52 of its 512 bytes per segment.
struct MetricsLayout { size_t totals, base0, seg_heads, base14, masks, bytes; };
static MetricsLayout metrics_layout(size_t n) {
  const RunsLayout R = runs_layout(n);
  const size_t cap = runs_nseg(n);
  static_assert(kMetricRows * sizeof(u32) + (kMetricRows - 1) * sizeof(u64) <= sizeof(RunStash) * kStashHeads, "the tables fit the stash region");
  MetricsLayout L;
  L.totals = R.totals;
  L.base0 = R.seg_base;
  L.base14 = R.stash;                                         // 16-byte aligned
  L.seg_heads = L.base14 + (kMetricRows - 1) * sizeof(u64) * cap;
  L.masks = R.mol_masks;
  L.bytes = R.mol_bytes;
  return L;
}
// run scratch: acc u64[16] | prefix u64[5][B] | verdict bytes
struct MetricsRunLayout { size_t prefix, verdict, bytes; };
static MetricsRunLayout metrics_run_layout(uint64_t nb) {
  const size_t b = nb ? nb : 1;
  MetricsRunLayout L;
  L.prefix = 128;
  L.verdict = L.prefix + kMetricRows * sizeof(u64) * b;
  L.bytes = align_up(L.verdict + b, 16);
  return L;
}
size_t metrics_scratch_bytes(size_t n) { return metrics_layout(n).bytes; }
size_t metrics_run_scratch_bytes(uint64_t barcodes) { return metrics_run_layout(barcodes).bytes; }

bool metrics_set_ok(const uint64_t* set, uint64_t set_bits, uint32_t set_word) {
  return (set_word == 1 || set_word == 2) && set_bits <= (1ull << 32) && (set || !set_bits) && (reinterpret_cast<uintptr_t>(set) & 7u) == 0;
}
bool metrics_limits_ok(const MetricsLimits& limits) {
  return limits.set_of <= 1 && limits.set_num <= limits.set_den && limits.set_den < (1ull << 24);
}

hipError_t launch_metrics_count(const LaunchCfg& cfg, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                                void* scratch, size_t scratch_bytes, hipStream_t st) {
  (void)hipGetLastError();
  const MetricsLayout L = metrics_layout(n);
  if (n == 0 || n >= (1ull << 40) || scratch_bytes < L.bytes || !metrics_set_ok(set, set_bits, set_word)) return hipErrorInvalidValue;
  const SegPlan sp = seg_plan(cfg, recs, n);
  u32* heads = scratch_at<u32>(scratch, L.seg_heads);
  hipLaunchKernelGGL(ibu_k_metrics_count, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, FeatureSet{(const u64*)set, (u64)set_bits, set_word}, heads);
  // the barcode row goes where launch_class_fill(ranked = false) reads its bases, the four others beside the counters
  launch_runs_scan(heads, sp.nseg, 1, scratch_at<u64>(scratch, L.base0), scratch_at<u64>(scratch, L.totals), st);
  launch_runs_scan(heads + sp.nseg, sp.nseg, kMetricRows - 1, scratch_at<u64>(scratch, L.base14), scratch_at<u64>(scratch, L.totals) + 1, st);
  return hipGetLastError();
}

// the emit pass of both entry points; masks: kept only when class bytes follow
static void metrics_emit(const LaunchCfg& cfg, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                         const void* scratch, void* run_scratch, uint64_t barcodes, uint64_t* d_barcodes, bool keep_masks, hipStream_t st) {
  const MetricsLayout L = metrics_layout(n);
  const SegPlan sp = seg_plan(cfg, recs, n);
  hipLaunchKernelGGL(ibu_k_metrics_emit, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, FeatureSet{(const u64*)set, (u64)set_bits, set_word},
                     scratch_at<const u64>(scratch, L.base0), scratch_at<const u64>(scratch, L.base14), (u64*)d_barcodes,
                     scratch_at<u64>(run_scratch, metrics_run_layout(barcodes).prefix), (u64)barcodes,
                     keep_masks ? scratch_at<u64>(scratch, L.masks) : nullptr);
}

hipError_t launch_metrics_table(const LaunchCfg& cfg, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                                const void* scratch, void* run_scratch, uint64_t barcodes, uint64_t* d_barcodes, uint64_t* d_reads,
                                uint64_t* d_pairs, uint64_t* d_triples, uint64_t* d_set_reads, uint64_t* d_set_triples, hipStream_t st) {
  (void)hipGetLastError();
  if (barcodes == 0 || barcodes > n || n >= (1ull << 40) || !metrics_set_ok(set, set_bits, set_word)) return hipErrorInvalidValue;
  metrics_emit(cfg, recs, n, set, set_bits, set_word, scratch, run_scratch, barcodes, d_barcodes, false, st);
  if (d_reads || d_pairs || d_triples || d_set_reads || d_set_triples)
    hipLaunchKernelGGL(ibu_k_metrics_table, dim3(capped_grid(cfg, barcodes, kSortThreads)), dim3(kSortThreads), 0, st,
                       scratch_at<const u64>(run_scratch, metrics_run_layout(barcodes).prefix), (u64)barcodes, (u64)n,
                       scratch_at<const u64>(scratch, metrics_layout(n).totals), (u64*)d_reads, (u64*)d_pairs, (u64*)d_triples, (u64*)d_set_reads,
                       (u64*)d_set_triples);
  return hipGetLastError();
}

hipError_t launch_metrics_filter(const LaunchCfg& cfg, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                                 void* scratch, void* run_scratch, uint64_t barcodes, const MetricsLimits& limits, uint8_t* d_class,
                                 hipStream_t st) {
  (void)hipGetLastError();
  if (barcodes == 0 || barcodes > n || n >= (1ull << 40) || !metrics_set_ok(set, set_bits, set_word) || !metrics_limits_ok(limits))
    return hipErrorInvalidValue;
  const MetricsRunLayout L = metrics_run_layout(barcodes);
  u64* acc = static_cast<u64*>(run_scratch);
  uint8_t* verdict = d_class ? scratch_at<uint8_t>(run_scratch, L.verdict) : nullptr;
  const hipError_t e = hipMemsetAsync(acc, 0, L.prefix, st);
  if (e != hipSuccess) return e;
  metrics_emit(cfg, recs, n, set, set_bits, set_word, scratch, run_scratch, barcodes, nullptr, d_class != nullptr, st);
  hipLaunchKernelGGL(ibu_k_metrics_verdict, dim3(capped_grid(cfg, barcodes, kSortThreads)), dim3(kSortThreads), 0, st,
                     scratch_at<const u64>(run_scratch, L.prefix), (u64)barcodes, (u64)n, scratch_at<const u64>(scratch, metrics_layout(n).totals),
                     limits, verdict, acc);
  if (d_class) return launch_class_fill(cfg, recs, n, scratch, false, verdict, d_class, st);
  return hipGetLastError();
}

}  // namespace ibu
