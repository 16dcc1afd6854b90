// k_cells.hip — ibu_call_cells: which barcodes of SORTED records are cells.  A barcode is a run of equal w0, its metric the (barcode,
// umi) pairs of the run (or its records); one integer threshold T decides, and T is a constant, the metric of the K-th largest
// barcode, or a tenth of the metric at the 99th percentile of the expected cells — include/ibu_hip.h has the rule in full.  The
// records are read twice and nothing goes to the host between the steps:
//   count    launch_runs_count(RunsCount::Barcode) of k_aggregate.hip, as for ibu_barcode_counts: barcodes and pairs per segment,
//            scanned; the two totals go back to the host to size the barcode table.
//   emit     the D = 1 walk of runs_walk.hpp again, with CellEmit as its sink: starts[b] = first row of barcode b, rank[b] = the pairs
//            that begin in front of it (16 bytes per barcode), and, when class bytes are wanted, the walk's ballots of RUN heads (16
//            bytes per 128-record tile) — the fill pass needs nothing else of the records.
//   table    metric[b] = rank[b + 1] - rank[b] (or starts[b + 1] - starts[b]): 8 bytes per barcode.
//   select   (TOP, ORDMAG) the r-th largest of the B metrics, all below 2^40, by MSB-first radix selection: five digit passes of
//            ibu_k_select_hist (the values that still match the prefix, counted by their next digit in an LDS histogram per workgroup,
//            one global atomic per non-empty bin and workgroup) and ibu_k_select_narrow (one workgroup walks the 256 bins from the
//            top and narrows prefix and remaining rank in device memory).  launch_rank_select is the same on any array of values.
//   verdict  one byte per barcode (metric >= T: 0, else 1) and the five sums, per wave with shuffles, per block in LDS, five atomics
//            per block of a grid that is capped.
//   fill     launch_class_fill of k_aggregate.hip: the ballots and the run heads' bases give each record's barcode number, the
//            verdicts leave as class bytes.
// Launchers: launch_cells_call, launch_rank_select (kernels.h); C ABI: ibu_call_cells (api_analysis.cpp; its test hook ibu_test_rank_select runs the selection alone).
#include "runs_walk.hpp"

namespace ibu {

static constexpr u32 kCellItems = 4;
static constexpr u32 kCellBlock = kSortThreads * kCellItems;  // barcodes per verdict round of a workgroup
static constexpr u32 kSelectPasses = 5;                       // 8-bit digits of a value below 2^40
static constexpr u32 kSelectBins = 256;
static_assert(kSelectBins == (u32)kSortThreads, "ibu_k_select_hist / _narrow: one thread per bin");

struct CellEmit : BallotSink {                                // keeps the ballots of run heads
  u64* starts; u64* rank;
  __device__ __forceinline__ void head(u64 b, u64 q, u64 row, u64, u64, bool run_head) const {
    if (!run_head) return;
    starts[b] = row;                                          // first record of barcode b
    rank[b] = q;                                              // (barcode, umi) pairs that begin in front of it
  }
  __device__ __forceinline__ void ballots(u64 at, bool tiled, u64 run_even, u64 run_odd, u64, u64) const { keep(at, tiled, run_even, run_odd); }
};
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_cells_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/, u64* __restrict__ starts,
                 u64* __restrict__ rank, u64* __restrict__ masks /*nullable*/) {
  runs_kernel<1>(recs, sp, seg_base, nullptr, CellEmit{{{}, masks}, starts, rank});
}

extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_cells_table(const u64* __restrict__ starts, const u64* __restrict__ rank, u64 nb, u64 n, u64 npairs, u32 by_reads, u64* __restrict__ metric) {
  const u64* src = by_reads ? starts : rank;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) metric[b] = closed_diff(src, b, nb, by_reads ? n : npairs);
}

// ---- rank selection: state u64[2] = (prefix: the digits decided so far, the rank that remains among the values under that prefix)
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_select_hist(const u64* __restrict__ values, u64 count, u32 pass, const u64* __restrict__ state, u64* __restrict__ hist /*[kSelectBins] of this pass*/) {
  __shared__ u32 bins[kSelectBins];
  bins[threadIdx.x] = 0;                                      // (kSortThreads == kSelectBins)
  __syncthreads();
  const u32 shift = 8 * (kSelectPasses - 1 - pass);
  const u64 prefix = pass ? state[0] : 0;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const u64 rounds = (count + stride - 1) / stride;             // the same for every wave: the ballot below wants whole waves
  for (u64 i = 0; i < rounds; ++i) {
    const u64 k = i * stride + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 bin = kSelectBins;                                    // nothing: past the end, or another prefix
    if (k < count) {
      const u64 v = values[k];
      if (!pass || (v >> (shift + 8)) == prefix) bin = (u32)(v >> shift) & (kSelectBins - 1);
    }
    const u32 first = __builtin_amdgcn_readfirstlane(bin);
    if (__ballot(bin != first) == 0) {                        // wave-uniform: one digit in all 64 values (equal metrics) is one add
      if (lane == 0 && first < kSelectBins) atomicAdd(&bins[first], (u32)kWave);
    } else if (bin < kSelectBins) {
      atomicAdd(&bins[bin], 1u);
    }
  }
  __syncthreads();
  const u32 c = bins[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], (u64)c);
}
// One workgroup: thread t holds bin 255 - t, so that an inclusive scan counts the values at or above a bin.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_select_narrow(const u64* __restrict__ hist /*[kSelectBins] of this pass*/, u32 pass, u64 rank0, u64* __restrict__ state) {
  __shared__ u64 wsum[kSortWaves];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 bin = kSelectBins - 1 - threadIdx.x;
  const u64 prefix = pass ? state[0] : 0, r = pass ? state[1] : rank0;
  const u64 c = hist[bin];
  u64 inc = wave_scan(c, OpAdd{});
  if (lane == kWave - 1) wsum[wib] = inc;
  __syncthreads();                                            // (also: every thread has read the state before one of them writes it)
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w)
    if ((u32)w < wib) inc += wsum[w];
  const u64 above = inc - c;                                  // values under the prefix with a larger digit
  if (above < r && r <= inc) { state[0] = (prefix << 8) | bin; state[1] = r - above; }
}

// acc (block_accumulate): [0] cells, [1] reads of cells, [2] of background, [3] umis of cells, [4] of background, [5] threshold, [6] baseline
// mode / param as in ibu_call_cells; selected: state[0] of the selection (TOP, ORDMAG), the metric at the rank asked for.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_cells_verdict(const u64* __restrict__ starts, const u64* __restrict__ rank, const u64* __restrict__ metric, u64 nb, u64 n, u64 npairs,
                    u32 mode, u64 param, const u64* __restrict__ selected, uint8_t* __restrict__ verdict /*nullable*/, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves * 5];
  const u64 value = mode == 0 ? 0 : selected[0];
  const u64 baseline = mode == 2 ? value : 0;
  const u64 T = mode == 0 ? param : mode == 1 ? value : (value + 9) / 10;
  if (blockIdx.x == 0 && threadIdx.x == 0) { acc[5] = T; acc[6] = baseline; }
  u64 t[5] = {0, 0, 0, 0, 0};
  for (u64 base = (u64)blockIdx.x * kCellBlock; base < nb; base += (u64)gridDim.x * kCellBlock) {   // (block-uniform)
    const u64 b0 = base + kCellItems * threadIdx.x;
    u64 s[kCellItems + 1], q[kCellItems + 1];
#pragma unroll
    for (u32 j = 0; j <= kCellItems; ++j) {
      s[j] = b0 + j < nb ? starts[b0 + j] : n;
      q[j] = b0 + j < nb ? rank[b0 + j] : npairs;
    }
    u32 packed = 0;
#pragma unroll
    for (u32 j = 0; j < kCellItems; ++j) {
      if (b0 + j < nb) {
        const bool cell = metric[b0 + j] >= T;
        const u64 reads = s[j + 1] - s[j], umis = q[j + 1] - q[j];
        packed |= (cell ? 0u : 1u) << (8 * j);
        t[0] += cell ? 1 : 0;
        t[1] += cell ? reads : 0;
        t[2] += cell ? 0 : reads;
        t[3] += cell ? umis : 0;
        t[4] += cell ? 0 : umis;
      }
    }
    if (verdict && b0 < nb) *reinterpret_cast<u32*>(verdict + b0) = packed;   // (the array is padded to a multiple of four)
  }
  block_accumulate(t, acc, accl);
}

// selection work: state u64[2] | .. 64: hist u64[kSelectPasses][kSelectBins]
static constexpr size_t kSelectHist = 64;
size_t rank_select_work_bytes() { return kSelectHist + sizeof(u64) * kSelectPasses * kSelectBins; }
hipError_t launch_rank_select(const LaunchCfg& cfg, const uint64_t* values, uint64_t count, uint64_t rank, void* work, hipStream_t st) {
  (void)hipGetLastError();
  if (count == 0 || rank == 0 || rank > count) return hipErrorInvalidValue;
  u64* state = static_cast<u64*>(work);
  u64* hist = scratch_at<u64>(work, kSelectHist);
  hipError_t e = hipMemsetAsync(work, 0, rank_select_work_bytes(), st);
  if (e != hipSuccess) return e;
  const u32 grid = capped_grid(cfg, count, 8 * kSortThreads);
  for (u32 pass = 0; pass < kSelectPasses; ++pass) {
    hipLaunchKernelGGL(ibu_k_select_hist, dim3(grid), dim3(kSortThreads), 0, st, (const u64*)values, (u64)count, pass, (const u64*)state,
                       hist + pass * kSelectBins);
    hipLaunchKernelGGL(ibu_k_select_narrow, dim3(1), dim3(kSortThreads), 0, st, (const u64*)(hist + pass * kSelectBins), pass, (u64)rank, state);
  }
  return hipGetLastError();
}

// run scratch: acc u64[8] | selection work | starts u64[B] | rank u64[B] | metric u64[B] | verdict bytes
struct CellLayout { size_t select, starts, rank, metric, verdict, bytes; };
static CellLayout cell_layout(uint64_t nb) {
  const size_t b = nb ? nb : 1;
  CellLayout L;
  L.select = 64;
  L.starts = align_up(L.select + rank_select_work_bytes(), 16);
  L.rank = L.starts + 8 * b;
  L.metric = L.rank + 8 * b;
  L.verdict = L.metric + 8 * b;
  L.bytes = align_up(L.verdict + b + 4, 16);
  return L;
}
size_t cells_run_scratch_bytes(uint64_t barcodes) { return cell_layout(barcodes).bytes; }
size_t cells_scratch_bytes(size_t n) { return runs_layout(n).mol_bytes; }
hipError_t launch_cells_call(const LaunchCfg& cfg, const void* recs, size_t n, void* scratch, void* run_scratch, uint64_t barcodes,
                             uint64_t pairs, uint32_t mode, uint64_t param, bool by_reads, uint8_t* d_class, hipStream_t st) {
  (void)hipGetLastError();
  if (barcodes == 0 || barcodes > n || pairs < barcodes || pairs > n || n >= (1ull << 40) || mode > 2 || (mode && !param))
    return hipErrorInvalidValue;
  const SegPlan sp = seg_plan(cfg, recs, n);
  const RunsLayout R = runs_layout(n);
  const u64* base = scratch_at<const u64>(scratch, R.seg_base);
  u64* masks = d_class ? scratch_at<u64>(scratch, R.mol_masks) : nullptr;
  const CellLayout L = cell_layout(barcodes);
  u64* acc = static_cast<u64*>(run_scratch);
  void* work = scratch_at<void>(run_scratch, L.select);
  u64* starts = scratch_at<u64>(run_scratch, L.starts);
  u64* rank = scratch_at<u64>(run_scratch, L.rank);
  u64* metric = scratch_at<u64>(run_scratch, L.metric);
  uint8_t* verdict = d_class ? scratch_at<uint8_t>(run_scratch, L.verdict) : nullptr;
  hipError_t e = hipMemsetAsync(acc, 0, 64, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ibu_k_cells_emit, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, base, starts, rank, masks);
  hipLaunchKernelGGL(ibu_k_cells_table, dim3(capped_grid(cfg, barcodes, kSortThreads)), dim3(kSortThreads), 0, st, (const u64*)starts,
                     (const u64*)rank, (u64)barcodes, (u64)n, (u64)pairs, by_reads ? 1u : 0u, metric);
  if (mode) {
    // TOP: the K-th largest (the smallest when there are fewer); ORDMAG: the 99th percentile of the top min(E, B), no interpolation
    const u64 top = param < barcodes ? param : barcodes;
    e = launch_rank_select(cfg, reinterpret_cast<const uint64_t*>(metric), barcodes, mode == 1 ? top : top / 100 + 1, work, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ibu_k_cells_verdict, dim3(capped_grid(cfg, barcodes, kCellBlock)), dim3(kSortThreads), 0, st, (const u64*)starts,
                     (const u64*)rank, (const u64*)metric, (u64)barcodes, (u64)n, (u64)pairs, mode, (u64)param, (const u64*)work, verdict, acc);
  if (d_class) return launch_class_fill(cfg, recs, n, scratch, false, verdict, d_class, st);
  return hipGetLastError();
}

}  // namespace ibu
