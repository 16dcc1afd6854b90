// k_partition.hip — stable multi-way partition of 24-byte records by class byte (include/ibu_hip.h: ibu_partition_records).
//
// Select's chain (k_whitelist.hip) with a part dimension: count -> scan -> scatter over UNITS of consecutive records, a unit
// belonging to one wave, so nothing here needs a workgroup barrier outside the one-workgroup scan.  The plan (unit size, table
// layout, scratch bytes) is host arithmetic in partition_plan.hpp.  The table is part-major — table[1 + p * nunits + u] — so ONE
// exclusive scan of the flattened table (scan_units_in_place, kcommon.hpp) turns the counts into the final output position of every
// (part, unit): part 0's units first, then part 1's.  table[0] is the total and table[1 + p * nunits] the start of part p.
//
// The 256-byte class -> part map travels as a kernel argument (PartitionMap) and every wave keeps a copy in its LDS slice, beside
// its counters: u32 counts per part (count), u64 running positions per part (scatter).  A wave's DS instructions execute in order,
// so the slice needs wave_lds_fence only.
#include "kcommon.hpp"
#include "kernels.h"
#include "partition_plan.hpp"

namespace ibu {

static constexpr u32 kPartSlots = 256;        // counters per wave: a slot per part byte (slot 255, "none", is never touched)
static constexpr u32 kPartChunk = 4;          // rounds of 64 records whose loads are issued together
static_assert(kPartitionMinUnit % (kWave * kPartChunk) == 0, "a unit is a whole number of chunks");

// The wave's copy of the map: 64 words, lane L brings word L.
__device__ __forceinline__ void part_map_load(u32* wmap, const PartitionMap& map, u32 lane) {
  wmap[lane] = map.w[lane];
  wave_lds_fence();
}
__device__ __forceinline__ u32 part_of_class(const u32* wmap, u32 c) { return reinterpret_cast<const uint8_t*>(wmap)[c]; }

// One count into the wave's histogram, as hist_add of sort_passes.hpp: class bytes arrive in long runs on sorted input, and 64
// lanes adding to one LDS word would take 64 turns — when all active lanes hold one part, one lane adds for all of them.
__device__ __forceinline__ void part_hist_add(u32* h, u32 p, bool active) {
  if (active) {
    const u32 f = (u32)__builtin_amdgcn_readfirstlane((int)p);
    if (__ballot(p != f) == 0) {                               // wave-uniform
      const u64 act = __ballot(true);
      if ((threadIdx.x & (kWave - 1)) == (u32)__ffsll((long long)act) - 1u) atomicAdd(&h[f], (u32)__popcll(act));
    } else {
      atomicAdd(&h[p], 1u);
    }
  }
}

// table[1 + p * nunits + u] = the records of unit u that go to part p
extern "C" __global__ void __launch_bounds__(kBlock, 4)
ibu_k_partition_count(const uint8_t* __restrict__ cls, u64 n, u32 unit, u32 nunits, u32 n_parts, const PartitionMap map,
                      u64* __restrict__ table) {
  __shared__ u32 s_map[kWavesPerBlock][kWave];
  __shared__ u32 s_hist[kWavesPerBlock][kPartSlots];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 nwaves = gridDim.x * kWavesPerBlock, rounds = unit / kWave;
  u32* wmap = s_map[wib];
  u32* h = s_hist[wib];
  part_map_load(wmap, map, lane);
  for (u32 u = blockIdx.x * kWavesPerBlock + wib; u < nunits; u += nwaves) {   // wave-uniform
#pragma unroll
    for (u32 k = 0; k < kPartSlots / kWave; ++k) h[lane + kWave * k] = 0;
    wave_lds_fence();
    const u64 first = (u64)u * unit + lane;
    for (u32 r = 0; r < rounds; r += kPartChunk) {
      u32 c[kPartChunk];
#pragma unroll
      for (u32 k = 0; k < kPartChunk; ++k) {
        const u64 i = first + (u64)(r + k) * kWave;
        c[k] = i < n ? (u32)cls[i] : 256u;
      }
#pragma unroll
      for (u32 k = 0; k < kPartChunk; ++k) {
        const u32 p = c[k] < 256u ? part_of_class(wmap, c[k]) : kPartitionNone;
        part_hist_add(h, p, p != kPartitionNone);
      }
    }
    wave_lds_fence();
    for (u32 p = lane; p < n_parts; p += kWave) table[1 + (u64)p * nunits + u] = h[p];
    wave_lds_fence();                                          // the next unit clears what these lanes read
  }
}

// One workgroup of kScanBlock threads: the exclusive scan of the flattened table, then the n_parts part starts and the total to
// starts[0 .. n_parts] for the read-back (starts lies behind the table).
extern "C" __global__ void __launch_bounds__(kScanBlock)
ibu_k_partition_scan(u64* __restrict__ table, u32 entries, u32 nunits, u32 n_parts, u64* __restrict__ starts) {
  scan_units_in_place(table, entries);
  __syncthreads();                                             // the scanned table, written by other threads of this workgroup
  if (threadIdx.x <= n_parts) starts[threadIdx.x] = threadIdx.x < n_parts ? table[1 + (u64)threadIdx.x * nunits] : table[0];
}

// A unit's kept records to their parts, in input order.  Per round of 64 records: the lanes that hold the same part find each
// other (match_digit), all read the part's running position, and the first of them moves it on.
extern "C" __global__ void __launch_bounds__(kBlock, 4)
ibu_k_partition_scatter(const u64* __restrict__ recs, const uint8_t* __restrict__ cls, u64 n, u32 unit, u32 nunits, u32 n_parts,
                        const PartitionMap map, const u64* __restrict__ table, u64* __restrict__ out) {
  __shared__ u32 s_map[kWavesPerBlock][kWave];
  __shared__ u64 s_pos[kWavesPerBlock][kPartSlots];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  const u32 nwaves = gridDim.x * kWavesPerBlock, rounds = unit / kWave;
  u32* wmap = s_map[wib];
  u64* pos = s_pos[wib];
  part_map_load(wmap, map, lane);
  for (u32 u = blockIdx.x * kWavesPerBlock + wib; u < nunits; u += nwaves) {   // wave-uniform
    wave_lds_fence();                                          // the previous unit's reads precede these writes
    for (u32 p = lane; p < n_parts; p += kWave) pos[p] = table[1 + (u64)p * nunits + u];
    wave_lds_fence();
    const u64 first = (u64)u * unit + lane;
    for (u32 r = 0; r < rounds; r += kPartChunk) {
      u32 c[kPartChunk], part[kPartChunk];
      u64 x[kPartChunk], y[kPartChunk], z[kPartChunk], dst[kPartChunk];
#pragma unroll
      for (u32 k = 0; k < kPartChunk; ++k) {
        const u64 i = first + (u64)(r + k) * kWave;
        c[k] = i < n ? (u32)cls[i] : 256u;
      }
#pragma unroll
      for (u32 k = 0; k < kPartChunk; ++k) {                   // the records' loads are in flight while the positions are worked out
        part[k] = c[k] < 256u ? part_of_class(wmap, c[k]) : kPartitionNone;
        x[k] = y[k] = z[k] = 0;
        if (part[k] != kPartitionNone) {
          const u64* s = recs + 3 * (first + (u64)(r + k) * kWave);
          x[k] = __builtin_nontemporal_load(s); y[k] = __builtin_nontemporal_load(s + 1); z[k] = __builtin_nontemporal_load(s + 2);
        }
      }
#pragma unroll
      for (u32 k = 0; k < kPartChunk; ++k) {
        const bool keep = part[k] != kPartitionNone;
        const DigitPeers pe = match_digit(part[k], __ballot(keep));
        const u64 prev = keep ? pos[part[k]] : 0;
        wave_lds_fence();                                      // every lane has read before the leaders write
        if (keep && pe.before == 0) pos[part[k]] = prev + pe.count;
        wave_lds_fence();
        dst[k] = prev + pe.before;
      }
#pragma unroll
      for (u32 k = 0; k < kPartChunk; ++k)
        if (part[k] != kPartitionNone) {
          u64* d = out + 3 * dst[k];
          __builtin_nontemporal_store(x[k], d); __builtin_nontemporal_store(y[k], d + 1); __builtin_nontemporal_store(z[k], d + 2);
        }
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
hipError_t launch_partition_count(const LaunchCfg& cfg, const uint8_t* d_class, size_t n, uint32_t n_parts, const PartitionMap& map,
                                  void* scratch, size_t scratch_bytes, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const PartitionPlan pl = partition_plan(n, n_parts);
  if (!pl.ok || scratch_bytes < pl.scratch_bytes) return hipErrorInvalidValue;
  u64* table = (u64*)scratch;
  static std::atomic<int> occ;
  hipLaunchKernelGGL(ibu_k_partition_count, dim3(grid_for((u32)pl.nunits, cfg.cus, resident_blocks<kBlock>(cfg, ibu_k_partition_count, 0, &occ))),
                     dim3(kBlock), 0, st, d_class, (u64)n, pl.unit, (u32)pl.nunits, n_parts, map, table);
  hipLaunchKernelGGL(ibu_k_partition_scan, dim3(1), dim3(kScanBlock), 0, st, table, (u32)pl.entries, (u32)pl.nunits, n_parts,
                     table + 1 + pl.entries);
  return hipGetLastError();
}
hipError_t launch_partition_scatter(const LaunchCfg& cfg, const void* recs, const uint8_t* d_class, size_t n, uint32_t n_parts,
                                    const PartitionMap& map, const void* scratch, void* out, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const PartitionPlan pl = partition_plan(n, n_parts);
  if (!pl.ok) return hipErrorInvalidValue;
  static std::atomic<int> occ;
  hipLaunchKernelGGL(ibu_k_partition_scatter, dim3(grid_for((u32)pl.nunits, cfg.cus, resident_blocks<kBlock>(cfg, ibu_k_partition_scatter, 0, &occ))),
                     dim3(kBlock), 0, st, (const u64*)recs, d_class, (u64)n, pl.unit, (u32)pl.nunits, n_parts, map, (const u64*)scratch,
                     (u64*)out);
  return hipGetLastError();
}

}  // namespace ibu
