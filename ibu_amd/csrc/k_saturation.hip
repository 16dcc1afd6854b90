// k_saturation.hip — ibu_subsample_class and ibu_saturation_curve: a reproducible random subset of the reads, and what would have been
// seen at K sequencing depths, from ONE read of the sorted records.  Both rest on the number of a read, u(row) = splitmix64(base + row)
// with base = splitmix64(seed) + first_row (the host adds the two): a pure function of the row, the record's contents do not enter.  A
// read is kept at threshold t iff u < t (t all ones keeps everything); a run (a barcode: equal w0, a molecule: equal (w0, w1)) is kept
// iff the smallest u among its reads is — include/ibu_hip.h has the rule in full.  With the K thresholds sorted, the BIN of a read is
// the number of thresholds <= u, 0 .. K: it is kept at point j iff bin <= j, a run's bin is the minimum over its reads, and the whole
// curve is three histograms over the bins, read cumulatively.
//   walk     the D = 1 walk of runs_walk.hpp (its run heads are barcode heads, its ranked heads molecule heads) with SatSink: per
//            128-record step the two bins of every lane (one splitmix64 and a search of at most six steps in the thresholds, kept in LDS), one
//            segmented min-scan over the wave for both depths at once (nine bits each in one word, six shuffles), the open run's
//            minimum carried in a register from tile to tile.  A run that begins and ends inside the segment is tallied there; the
//            tally is bit-sliced — a ballot per bit of the bins, lane j keeps the count of bin j — so there is no atomic and no
//            LDS histogram.  The segment leaves 3 x 33 counters, and for each depth (leading min, has a head, trailing min).
//   sum      the segments' counters added up: coalesced rows, one atomic per workgroup and bin.
//   stitch   one workgroup per depth runs an exclusive segmented min-scan over the segments' summaries, 1024 per round: a segment with
//            a head closes the run that comes in (carry joined with its leading min), the run open at the end of the data closes
//            there.  A run over all of 1e9 records is 122 071 scan entries, 120 rounds: the cost does not depend on run lengths.
//   points   the 3 x K cumulative counts.
// The subsample writes one class byte per row, sixteen rows per lane and dwordx4 store where the class array's alignment allows, bytes at
// its two ends; the kept count goes through block_accumulate, one atomic per workgroup.
// Launchers: launch_subsample, launch_saturation (kernels.h); C ABI: ibu_subsample_class, ibu_saturation_curve (api_analysis.cpp).
#include "runs_walk.hpp"

namespace ibu {

static constexpr u32 kSatBins = kSaturationMaxPoints + 1;     // bins 0 .. 32
static constexpr u32 kSatNone = 64;                           // the minimum of no read: above every bin, fits the 8-bit field
static constexpr u32 kSatRow = 100;                           // u32 per segment: reads[33] | barcodes[33] | molecules[33] | unused
static constexpr u32 kSatFlag = 0x100;                        // (flag << 8 | min): one depth of a scan element
static constexpr u32 kSatSearch = 64;                         // thresholds in LDS, padded with all ones: a fixed six-step search

// a in front of b; the flag says that a run head lies in the stretch, the min is the one behind the last head (of all of it without)
__device__ __forceinline__ u32 sat_join1(u32 a, u32 b) {
  const u32 av = a & 0xFFu, bv = b & 0xFFu;
  const u32 m = av < bv ? av : bv;
  return (b & kSatFlag) ? b : ((a & kSatFlag) | m);
}
// both depths in one word: bits 0-8 the barcode level, bits 16-24 the molecule level
__device__ __forceinline__ u32 sat_join(u32 a, u32 b) {
  return sat_join1(a & 0x1FFu, b & 0x1FFu) | (sat_join1((a >> 16) & 0x1FFu, (b >> 16) & 0x1FFu) << 16);
}
__device__ __forceinline__ u32 sat_min(u32 a, u32 b) { return a < b ? a : b; }

// The number of thresholds <= u, the all-ones threshold (which keeps everything) never counted.  T: kSatSearch entries, non-decreasing,
// all ones from entry K on; nbits: the bits of a bin, 2^nbits >= K + 1 (wave-uniform), so the answer lies below 2^nbits and the
// steps of a larger stride are skipped.
__device__ __forceinline__ u32 sat_bin(const u64* T, u64 u, u32 nbits) {
  u32 pos = 0;
#pragma unroll
  for (u32 i = 6; i-- > 0;) {
    if (i < nbits) {                                          // wave-uniform
      const u32 s = 1u << i;
      const u64 t = T[pos + s - 1];
      pos += (t <= u && t != ~0ull) ? s : 0;
    }
  }
  return pos;
}
// How many of the wave's valid lanes bring bin == lane: nbits ballots of the bins' bits, each lane keeps the lanes that agree with its
// own number in every one of them.  (A lane that is not valid may bring anything.  A lane at or above 2^nbits counts the bin of its
// low bits over again; those counters lie above bin K, which no point reads.)  Nothing valid — the rule for barcode heads, which
// are thousands of records apart — costs one ballot.
__device__ __forceinline__ u32 sat_tally(u32 bin, bool valid, u32 lane, u32 nbits) {
  u64 m = __ballot(valid);
  if (m == 0) return 0;                                       // wave-uniform
#pragma unroll
  for (u32 i = 0; i < 6; ++i) {
    if (i < nbits) {                                          // wave-uniform
      const u64 b = __ballot(((bin >> i) & 1u) != 0);
      m &= ((lane >> i) & 1u) ? b : ~b;
    }
  }
  return (u32)__popcll(m);
}

struct SatSink : NoSink {
  const u64* T;                                               // the wave's thresholds in LDS
  u64 base, end;                                              // u(row) = splitmix64(base + row); the first row behind the segment
  u32 lane, nbits;                                            // 2^nbits >= K + 1.  (its own lane and end, not WalkStep's lane and va: 82 VGPRs for 80 with those)
  // carried from step to step (wave-uniform but for `lead` and the tallies)
  mutable u32 open1, open2;                                   // the min of the run open at the end of the rows walked so far
  mutable u32 seen1, seen2;                                   // kSatFlag once the segment has had a head
  mutable u32 lead1, lead2;                                   // in the one lane that met the segment's first head: the min in front of it
  mutable u32 reads, runs1, runs2;                            // lane j: reads / closed runs of bin j
  __device__ __forceinline__ void step(const WalkStep& s) const {
    const u64 row = s.row;
    const bool va = row < end, a1 = s.a1, a2 = s.a2, b1 = s.b1, b2 = s.b2, pair = s.pair;
    const u32 ba = va ? sat_bin(T, splitmix64(base + row), nbits) : kSatNone;
    const u32 bb = pair ? sat_bin(T, splitmix64(base + row + 1), nbits) : kSatNone;
    reads += sat_tally(ba, va, lane, nbits);
    if (pair) reads += sat_tally(bb, true, lane, nbits);
    // the lane's own stretch (a, b) at both depths, then the inclusive scan over the wave
    const u32 both = sat_min(ba, bb);
    u32 x = (b1 ? bb | kSatFlag : a1 ? both | kSatFlag : both) | ((b2 ? bb | kSatFlag : a2 ? both | kSatFlag : both) << 16);
    x = wave_scan(x, [](u32 p, u32 v) { return sat_join(p, v); });
    u32 ex = __shfl_up(x, 1);
    if (lane == 0) ex = kSatNone | (kSatNone << 16);
    const u32 last = __shfl(x, kWave - 1);
    {                                                         // barcode level
      const u32 e = ex & 0x1FFu;
      const u32 in = (e & kSatFlag) ? (e & 0xFFu) : sat_min(open1, e & 0xFFu);   // the min of the run that is open in front of a
      const bool before = ((e | seen1) & kSatFlag) != 0;                        // a head of this segment lies in front of a
      runs1 += sat_tally(in, va && a1 && before, lane, nbits);
      if (va && a1 && !before) lead1 = in;
      if (pair) {
        const u32 inb = a1 ? ba : sat_min(in, ba);
        runs1 += sat_tally(inb, b1 && (before || a1), lane, nbits);
        if (b1 && !(before || a1)) lead1 = inb;
      }
      const u32 l = last & 0x1FFu;
      open1 = (l & kSatFlag) ? (l & 0xFFu) : sat_min(open1, l & 0xFFu);
      seen1 |= l & kSatFlag;
    }
    {                                                         // molecule level
      const u32 e = (ex >> 16) & 0x1FFu;
      const u32 in = (e & kSatFlag) ? (e & 0xFFu) : sat_min(open2, e & 0xFFu);
      const bool before = ((e | seen2) & kSatFlag) != 0;
      runs2 += sat_tally(in, va && a2 && before, lane, nbits);
      if (va && a2 && !before) lead2 = in;
      if (pair) {
        const u32 inb = a2 ? ba : sat_min(in, ba);
        runs2 += sat_tally(inb, b2 && (before || a2), lane, nbits);
        if (b2 && !(before || a2)) lead2 = inb;
      }
      const u32 l = (last >> 16) & 0x1FFu;
      open2 = (l & kSatFlag) ? (l & 0xFFu) : sat_min(open2, l & 0xFFu);
      seen2 |= l & kSatFlag;
    }
  }
};

// a segment's summary at one depth: leading min | trailing min << 8 | has a head << 16
__device__ __forceinline__ u32 sat_summary(u32 seen, u32 lead, u32 open) {
  return seen ? (lead | (open << 8) | (1u << 16)) : (open | (open << 8));
}

struct SatThresholds { u64 t[kSaturationMaxPoints]; };        // the entries behind the K given: all ones

extern "C" __global__ void __launch_bounds__(kSortThreads, 4)
ibu_k_saturation_walk(const u64* __restrict__ recs, SegPlan sp, SatThresholds th, u32 nbits, u64 base, u32* __restrict__ hist /*[nseg][kSatRow]*/,
                      u32* __restrict__ summary /*[nseg][2]*/) {
  __shared__ u64 search[kSortWaves][kSatSearch];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  u64 mine = ~0ull;
#pragma unroll
  for (u32 j = 0; j < kSaturationMaxPoints; ++j) mine = lane == j ? th.t[j] : mine;   // (static indices: the thresholds stay kernel arguments)
  search[wib][lane] = mine;
  wave_lds_fence();
  const u32 seg = wave_segment();
  const u64 stop = sp.head + sp.main, first = seg_first_row(sp, seg);
  const u64 end = seg == 0 ? sp.head : seg == sp.nseg - 1 ? sp.n : (first + kSegRecs < stop ? first + kSegRecs : stop);
  const SatSink sink{{}, search[wib], base, end, lane, nbits, kSatNone, kSatNone, 0, 0, kSatNone, kSatNone, 0, 0, 0};
  walk_wave<1>(recs, sp, nullptr, sink, [&](u32 seg, u32 lane, SegCounts) {   // (the walk's seg and lane from here on)
    const u32 lead1 = wave_reduce(sink.lead1, OpMin{}), lead2 = wave_reduce(sink.lead2, OpMin{});
    u32* row = hist + (size_t)seg * kSatRow;
    if (lane < kSatBins) {                                    // (the counters above bin K are never read: sat_tally)
      row[lane] = sink.reads;
      row[kSatBins + lane] = sink.runs1;
      row[2 * kSatBins + lane] = sink.runs2;
    }
    if (lane == 0) {
      summary[2 * (size_t)seg] = sat_summary(sink.seen1, lead1, sink.open1);
      summary[2 * (size_t)seg + 1] = sat_summary(sink.seen2, lead2, sink.open2);
    }
  });
}

// totals: u64[3][kSatBins] (reads, barcodes, molecules by bin), zeroed by the launcher
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_saturation_sum(const u32* __restrict__ hist, u32 nseg, u64* __restrict__ totals) {
  __shared__ u64 part[kSortThreads / 2];
  const u32 col = threadIdx.x & 127u, half = threadIdx.x >> 7;
  u64 s = 0;
  if (col < 3 * kSatBins)
    for (u64 seg = 2 * (u64)blockIdx.x + half; seg < nseg; seg += 2 * (u64)gridDim.x) s += hist[seg * kSatRow + col];
  if (half == 1) part[col] = s;
  __syncthreads();
  if (half == 0 && col < 3 * kSatBins) {
    s += part[col];
    if (s) atomicAdd(&totals[col], s);
  }
}

// One workgroup per depth (blockIdx.x).  Segment s enters the scan as a start with its trailing min when it has a head, and as its
// leading min (all of it) otherwise; what is open in front of s, joined with its leading min, is the run that s's first head closes.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_saturation_stitch(const u32* __restrict__ summary /*[nseg][2]*/, u32 nseg, u64* __restrict__ totals) {
  __shared__ u32 wv[kSortWaves];
  __shared__ u32 closed[kSatBins];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6, depth = blockIdx.x;
  if (threadIdx.x < kSatBins) closed[threadIdx.x] = 0;
  __syncthreads();
  u32 carry = kSatNone;                                       // the min of the run open behind the segments scanned so far
  for (u32 s_base = 0; s_base < nseg; s_base += 4 * kSortThreads) {   // (block-uniform trip count: the scan has barriers)
    const u32 s0 = s_base + 4 * threadIdx.x;
    u32 sm[4];
    u32 run = kSatNone;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
      sm[k] = s0 + k < nseg ? summary[2 * (size_t)(s0 + k) + depth] : (kSatNone | (kSatNone << 8));
      run = sat_join1(run, (sm[k] >> 16) ? (((sm[k] >> 8) & 0xFFu) | kSatFlag) : (sm[k] & 0xFFu));
    }
    const u32 inc = wave_scan(run, [](u32 p, u32 v) { return sat_join1(p, v); });
    if (lane == kWave - 1) wv[wib] = inc;
    __syncthreads();
    u32 in = carry, all = carry;                              // open in front of this wave / behind the last one
#pragma unroll
    for (u32 w = 0; w < (u32)kSortWaves; ++w) {
      all = sat_join1(all, wv[w]);
      if (w + 1 == wib) in = all;
    }
    __syncthreads();                                          // (wv is written again in the next round)
    carry = all & 0xFFu;
    u32 ex = __shfl_up(inc, 1);
    if (lane == 0) ex = kSatNone;
    u32 open = sat_join1(in, ex) & 0xFFu;                     // the min of the run open in front of this thread's segments
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
      const u32 lead = sm[k] & 0xFFu, trail = (sm[k] >> 8) & 0xFFu;
      if (sm[k] >> 16) {
        const u32 c = sat_min(open, lead);
        if (c < kSatBins) atomicAdd(&closed[c], 1u);           // (one per segment; kSatNone: the head is row 0, nothing ends there)
        open = trail;
      } else {
        open = sat_min(open, lead);
      }
    }
  }
  if (threadIdx.x == 0 && carry < kSatBins) atomicAdd(&closed[carry], 1u);   // the run open at the end of the data
  __syncthreads();
  if (threadIdx.x < kSatBins && closed[threadIdx.x]) atomicAdd(&totals[(1 + depth) * kSatBins + threadIdx.x], (u64)closed[threadIdx.x]);
}

// points: u64[3][kSaturationMaxPoints]; point j = the bins 0 .. j
extern "C" __global__ void __launch_bounds__(kWave)
ibu_k_saturation_points(const u64* __restrict__ totals, u32 k, u64* __restrict__ points) {
  const u32 j = threadIdx.x;
  if (j >= k) return;
#pragma unroll
  for (u32 r = 0; r < 3; ++r) {
    u64 s = 0;
    for (u32 b = 0; b <= j; ++b) s += totals[r * kSatBins + b];
    points[r * kSaturationMaxPoints + j] = s;
  }
}

// ---- the subsample: class byte 0 (kept) where u(row) < threshold or the threshold is all ones, 1 (dropped) elsewhere -------------
// `front` rows lie in front of the first 16-byte aligned class byte, `units` whole 16-row units behind them, fewer than 16 rows behind
// those.  d_class == nullptr: the count alone.  acc (nullable, uniform over the grid; block_accumulate): [0] the kept rows.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_subsample(u64 n, u64 base, u64 threshold, u64 front, u64 units, uint8_t* __restrict__ d_class, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves];
  const bool all = threshold == ~0ull;
  u32 kept = 0;
  const u64 stride = (u64)gridDim.x * kSortThreads;
  for (u64 unit = (u64)blockIdx.x * kSortThreads + threadIdx.x; unit < units; unit += stride) {
    const u64 r0 = front + 16 * unit;
    u32 w[4];
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
      w[q] = 0;
#pragma unroll
      for (u32 b = 0; b < 4; ++b) {
        const bool keep = all || splitmix64(base + r0 + 4 * q + b) < threshold;
        kept += keep ? 1u : 0u;
        w[q] |= (keep ? 0u : 1u) << (8 * b);
      }
    }
    if (d_class) { u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3]; st16(d_class + r0, v); }
  }
  if (blockIdx.x == 0 && threadIdx.x < 32) {                  // the two ends, a byte per lane
    const u64 i = threadIdx.x & 15u;
    const bool back = threadIdx.x >= 16;
    const u64 row = back ? front + 16 * units + i : i;
    if (back ? row < n : i < front) {
      const bool keep = all || splitmix64(base + row) < threshold;
      kept += keep ? 1u : 0u;
      if (d_class) d_class[row] = keep ? 0 : 1;
    }
  }
  if (!acc) return;                                           // (uniform)
  u64 t[1] = {kept};
  block_accumulate(t, acc, accl);
}

uint64_t sample_base(uint64_t seed, uint64_t first_row) { return splitmix64(seed) + first_row; }

hipError_t launch_subsample(const LaunchCfg& cfg, size_t n, uint64_t base, uint64_t threshold, uint8_t* d_class, uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0 || n >= (1ull << 40)) return hipErrorInvalidValue;
  const hipError_t e = zero_totals(acc, 1, st);
  if (e != hipSuccess) return e;
  u64 front = d_class ? (u64)((16 - (reinterpret_cast<uintptr_t>(d_class) & 15u)) & 15u) : 0;
  front = front < n ? front : n;
  const u64 units = (n - front) / 16;
  hipLaunchKernelGGL(ibu_k_subsample, dim3(capped_grid(cfg, units, kSortThreads)), dim3(kSortThreads), 0, st, (u64)n, (u64)base, (u64)threshold, front, units,
                     d_class, (u64*)acc);
  return hipGetLastError();
}

// scratch: totals u64[3][33] | 1024: points u64[3][32] | 2048: summary u32[cap][2] | hist u32[cap][kSatRow], cap = runs_nseg(n): a
// function of n alone, as runs_layout is, and indexed by the plan's segments, of which there are at most cap
struct SatLayout { size_t points, summary, hist, bytes; };
static SatLayout sat_layout(size_t n) {
  const size_t cap = runs_nseg(n);
  SatLayout L;
  L.points = 1024;
  L.summary = 2048;
  L.hist = align_up(L.summary + 2 * sizeof(u32) * cap, 16);
  L.bytes = L.hist + sizeof(u32) * kSatRow * cap;
  return L;
}
size_t saturation_scratch_bytes(size_t n) { return sat_layout(n).bytes; }
size_t saturation_points_offset() { return 1024; }
hipError_t launch_saturation(const LaunchCfg& cfg, const void* recs, size_t n, uint64_t base, const uint64_t* thresholds, uint32_t k, void* scratch,
                             size_t scratch_bytes, hipStream_t st) {
  (void)hipGetLastError();
  const SatLayout L = sat_layout(n);
  if (n == 0 || n >= (1ull << 40) || k == 0 || k > kSaturationMaxPoints || scratch_bytes < L.bytes) return hipErrorInvalidValue;
  SatThresholds th;
  for (u32 j = 0; j < kSaturationMaxPoints; ++j) th.t[j] = j < k ? thresholds[j] : ~0ull;
  const SegPlan sp = seg_plan(cfg, recs, n);
  u64* totals = static_cast<u64*>(scratch);
  u32* summary = scratch_at<u32>(scratch, L.summary);
  u32* hist = scratch_at<u32>(scratch, L.hist);
  const hipError_t e = hipMemsetAsync(totals, 0, L.points, st);
  if (e != hipSuccess) return e;
  u32 nbits = 1;
  while ((1u << nbits) < k + 1) ++nbits;                      // 1 .. 6
  hipLaunchKernelGGL(ibu_k_saturation_walk, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, th, nbits, (u64)base, hist, summary);
  // 32 rows or more per half workgroup
  hipLaunchKernelGGL(ibu_k_saturation_sum, dim3(capped_grid(cfg, sp.nseg, 64, 4)), dim3(kSortThreads), 0, st, (const u32*)hist, sp.nseg, totals);
  hipLaunchKernelGGL(ibu_k_saturation_stitch, dim3(2), dim3(kSortThreads), 0, st, (const u32*)summary, sp.nseg, totals);
  hipLaunchKernelGGL(ibu_k_saturation_points, dim3(1), dim3(kWave), 0, st, (const u64*)totals, k, scratch_at<u64>(scratch, L.points));
  return hipGetLastError();
}

}  // namespace ibu
