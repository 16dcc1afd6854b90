// k_matrix.hip — the matrix export (include/ibu_hip.h: ibu_matrix_rows, ibu_matrix_market_body).  Both calls work on the ENTRY TABLE,
// the u64 columns ibu_pair_counts / ibu_count_matrix leave, and both have the shape select has in k_whitelist.hip: a UNIT is 2048
// consecutive entries and belongs to one wave, a count pass leaves one u64 per unit, the single-workgroup scan of kcommon.hpp
// (scan_units_in_place) turns them into offsets with the total in front, and a scatter pass writes.  No workgroup barrier in the
// streaming kernels and no hand-off between workgroups inside a launch.
//   rows: what is counted is the HEADS, the entries whose value differs from the entry before (entry 0 is one); the offsets are row
//         ordinals.
//   text: what is counted is BYTES, the lengths of the decimal lines; the offsets are positions in the text.
// Scratch (matrix_scratch_bytes): u64 [0 .. 2] the maxima of the three printed columns (text only), [3] the total, [4 + u] unit u.
#include "kcommon.hpp"

#include "dec_format.hpp"

namespace ibu {

static constexpr u32 kMtxUnit = 2048, kMtxRounds = kMtxUnit / kWave;
static constexpr u32 kMtxHead = kMatrixTotalWord;  // scratch words in front of the scanned array (whose word 0 is the total)
static constexpr u32 kMtxStage = 4096;             // LDS bytes per wave: a round of 64 lines is at most 64 x 63 = 4032, plus the phase (< 4)

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const u32 lo = __shfl((u32)v, src), hi = __shfl((u32)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}

// ---- rows ------------------------------------------------------------------------------------------------------------
// The heads of one round: lane L looks at entry i = the round's first + L.  `carry`: the value in front of the round's first entry
// (lane 63 of the round before; at a unit's first entry, read from global memory by the caller).
__device__ __forceinline__ bool mtx_head(const u64* __restrict__ first, u64 i, u64 n, u32 lane, u64& carry, u64& cur) {
  cur = i < n ? __builtin_nontemporal_load(first + i) : 0;
  u64 prev = shfl_up64(cur, 1);
  if (lane == 0) prev = carry;
  carry = shfl64(cur, kWave - 1);
  return i < n && (i == 0 || cur != prev);
}

extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_matrix_rows_count(const u64* __restrict__ first, u64 n, u32 nunits, u64* __restrict__ units) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    const u64 base = (u64)u * kMtxUnit;
    u64 carry = base ? first[base - 1] : 0, cur;
    u32 k = 0;
#pragma unroll 4
    for (u32 r = 0; r < kMtxRounds; ++r) k += (u32)__builtin_popcountll(__ballot(mtx_head(first, base + r * kWave + lane, n, lane, carry, cur)));
    if (lane == 0) units[1 + u] = k;
  }
}

extern "C" __global__ void __launch_bounds__(kScanBlock)
ibu_k_matrix_scan(u64* __restrict__ units, u32 nunits) {
  scan_units_in_place(units, nunits);
}

// Each output is nullable.  row_ptr has units[0] + 1 words: the last is n, written by one lane of one wave.
extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_matrix_rows_scatter(const u64* __restrict__ first, u64 n, u32 nunits, const u64* __restrict__ units, u64* __restrict__ row_of_entry,
                          u64* __restrict__ row_keys, u64* __restrict__ row_ptr) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  const u64 upto = ~0ull >> (63 - lane);           // this lane and the lanes below it
  if (row_ptr && blockIdx.x == 0 && threadIdx.x == 0) row_ptr[units[0]] = n;
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    const u64 base = (u64)u * kMtxUnit;
    u64 carry = base ? first[base - 1] : 0, cur;
    u64 pos = units[1 + u];                        // heads in front of this unit
#pragma unroll 4
    for (u32 r = 0; r < kMtxRounds; ++r) {
      const u64 i = base + r * kWave + lane;
      const bool head = mtx_head(first, i, n, lane, carry, cur);
      const u64 b = __ballot(head);
      // entry 0 is a head, so every entry has one at or in front of it: the ordinal is never negative
      const u64 ord = pos + (u32)__builtin_popcountll(b & upto) - 1;
      if (i < n && row_of_entry) __builtin_nontemporal_store(ord, row_of_entry + i);
      if (head) {
        if (row_keys) row_keys[ord] = cur;
        if (row_ptr) row_ptr[ord] = i;
      }
      pos += (u32)__builtin_popcountll(b);
    }
  }
}

// ---- text ------------------------------------------------------------------------------------------------------------
// One line: the three printed values and their digit counts.  An entry past the end has length 0.
struct MtxLine {
  u64 a, b, c;
  u32 na, nb, nc, len;
};
__device__ __forceinline__ MtxLine mtx_line(const u64* __restrict__ pa, const u64* __restrict__ pb, const u64* __restrict__ pc, u64 i, u64 n,
                                            u64 add_a, u64 add_b) {
  MtxLine l;
  const bool in = i < n;
  l.a = in ? __builtin_nontemporal_load(pa + i) + add_a : 0;   // modulo 2^64
  l.b = in ? __builtin_nontemporal_load(pb + i) + add_b : 0;
  l.c = in ? __builtin_nontemporal_load(pc + i) : 0;
  if (__ballot(((l.a | l.b | l.c) >> 32) != 0) == 0)             // wave-uniform: the round holds no value of 2^32 or more
    l.na = dec_digits32((u32)l.a), l.nb = dec_digits32((u32)l.b), l.nc = dec_digits32((u32)l.c);
  else
    l.na = dec_digits(l.a), l.nb = dec_digits(l.b), l.nc = dec_digits(l.c);
  l.len = in ? l.na + l.nb + l.nc + 3 : 0;
  return l;
}

// units[1 + u] = the bytes of unit u's lines; maxima[0 .. 2] (zeroed by the launcher) = the largest printed value of each column,
// folded in with one integer atomic max per column and wave, when the wave leaves.  (Four waves per SIMD: four rounds
// in flight, three values each and both digit counters, do not fit the 64 registers of eight.)
extern "C" __global__ void __launch_bounds__(kBlock, 4)
ibu_k_matrix_text_count(const u64* __restrict__ pa, const u64* __restrict__ pb, const u64* __restrict__ pc, u64 n, u32 nunits, u64 add_a,
                        u64 add_b, u64* __restrict__ maxima, u64* __restrict__ units) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  u64 m[3] = {0, 0, 0};
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    u32 bytes = 0;                                 // at most 32 x 63 per lane
#pragma unroll 4
    for (u32 r = 0; r < kMtxRounds; ++r) {
      const MtxLine l = mtx_line(pa, pb, pc, (u64)u * kMtxUnit + r * kWave + lane, n, add_a, add_b);
      bytes += l.len;
      m[0] = l.a > m[0] ? l.a : m[0];
      m[1] = l.b > m[1] ? l.b : m[1];
      m[2] = l.c > m[2] ? l.c : m[2];
    }
    bytes = wave_reduce(bytes, OpAdd{});
    if (lane == 0) units[1 + u] = bytes;
  }
  wave_reduce(m, OpMax{});
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (m[k]) atomicMax(&maxima[k], m[k]);
}

// The decimal text of v, nd digits, ending just in front of stage[end].
__device__ __forceinline__ void mtx_put(uint8_t* stage, u32 end, u64 v, u32 nd) {
  dec_emit(v, nd, [stage, end](uint32_t k, char ch) { stage[end - 1 - k] = (uint8_t)ch; });
}

// Per round of 64 entries: wave_scan of the line lengths gives every lane its offset, the lane writes its line into the wave's LDS
// stage, and the wave copies the staged bytes out together — dword stores for the 4-byte aligned middle of its span of the text,
// byte stores for the up to three bytes at either end.  The bytes are staged at the PHASE of their destination (stage offset =
// text address modulo 4 + offset in the round), so an aligned dword of the text is an aligned dword of the stage.  No global dword
// that holds a byte of another wave, another round's neighbour or the caller is ever written: text may begin and end anywhere.
extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_matrix_text_write(const u64* __restrict__ pa, const u64* __restrict__ pb, const u64* __restrict__ pc, u64 n, u32 nunits, u64 add_a,
                        u64 add_b, const u64* __restrict__ units, uint8_t* __restrict__ text) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_all[kWavesPerBlock][kMtxStage];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  uint8_t* const stage = stage_all[threadIdx.x >> 6];
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    u64 pos = units[1 + u];                        // bytes of text in front of this unit
    for (u32 r = 0; r < kMtxRounds; ++r) {
      const u64 i0 = (u64)u * kMtxUnit + r * kWave;
      if (i0 >= n) break;                          // wave-uniform
      const MtxLine l = mtx_line(pa, pb, pc, i0 + lane, n, add_a, add_b);
      const u32 inc = wave_scan(l.len, OpAdd{});
      const u32 total = __shfl(inc, kWave - 1);    // 6 .. 4032
      uint8_t* const dst = text + pos;
      const u32 ph = (u32)(uintptr_t)dst & 3u;
      if (l.len) {
        u32 e = ph + inc - l.len + l.na;
        mtx_put(stage, e, l.a, l.na);
        stage[e] = ' ';
        e += 1 + l.nb;
        mtx_put(stage, e, l.b, l.nb);
        stage[e] = ' ';
        e += 1 + l.nc;
        mtx_put(stage, e, l.c, l.nc);
        stage[e] = '\n';
      }
      wave_lds_fence();
      // stage coordinates: the round's bytes are [ph, end); whole dwords [4 w0, 4 w1); what is left at either end goes out as bytes
      const u32 end = ph + total;
      const u32 w0 = (ph + 3) >> 2, w1 = end >> 2;
      const u32 head_end = 4 * w0 < end ? 4 * w0 : end;
      const u32 tail_at = 4 * w1 > head_end ? 4 * w1 : head_end;
      uint8_t* const gbase = dst - ph;             // 4-byte aligned; only bytes at or behind dst are written
      if (ph + lane < head_end) gbase[ph + lane] = stage[ph + lane];
      if (tail_at + lane < end) gbase[tail_at + lane] = stage[tail_at + lane];
      for (u32 w = w0 + lane; w < w1; w += kWave)
        __builtin_nontemporal_store(*reinterpret_cast<const u32*>(stage + 4 * w), reinterpret_cast<u32*>(gbase + 4 * (size_t)w));
      wave_lds_fence();                            // the next round overwrites the stage
      pos += total;
    }
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
static inline u64 mtx_units(size_t n) { return (n + kMtxUnit - 1) / kMtxUnit; }
size_t matrix_scratch_bytes(size_t n) { return 8 * (kMtxHead + 1 + mtx_units(n)); }
static inline u64* mtx_scan_array(const void* scratch) { return (u64*)scratch + kMtxHead; }

hipError_t launch_matrix_rows_count(const LaunchCfg& cfg, const uint64_t* first, size_t n, void* scratch, size_t scratch_bytes, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = mtx_units(n);
  if (nunits > 0xFFFFFFFFull || scratch_bytes < matrix_scratch_bytes(n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ibu_k_matrix_rows_count, dim3(tiled_grid<ibu_k_matrix_rows_count>(cfg, (u32)nunits)), dim3(kBlock), 0, st, (const u64*)first,
                     (u64)n, (u32)nunits, mtx_scan_array(scratch));
  hipLaunchKernelGGL(ibu_k_matrix_scan, dim3(1), dim3(kScanBlock), 0, st, mtx_scan_array(scratch), (u32)nunits);
  return hipGetLastError();
}
hipError_t launch_matrix_rows_scatter(const LaunchCfg& cfg, const uint64_t* first, size_t n, const void* scratch, uint64_t* row_of_entry,
                                      uint64_t* row_keys, uint64_t* row_ptr, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = mtx_units(n);
  hipLaunchKernelGGL(ibu_k_matrix_rows_scatter, dim3(tiled_grid<ibu_k_matrix_rows_scatter>(cfg, (u32)nunits)), dim3(kBlock), 0, st,
                     (const u64*)first, (u64)n, (u32)nunits, (const u64*)mtx_scan_array(scratch), (u64*)row_of_entry, (u64*)row_keys, (u64*)row_ptr);
  return hipGetLastError();
}
hipError_t launch_matrix_text_count(const LaunchCfg& cfg, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n, uint64_t add_a,
                                    uint64_t add_b, void* scratch, size_t scratch_bytes, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = mtx_units(n);
  if (nunits > 0xFFFFFFFFull || scratch_bytes < matrix_scratch_bytes(n)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(scratch, 0, 8 * kMtxHead, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ibu_k_matrix_text_count, dim3(tiled_grid<ibu_k_matrix_text_count>(cfg, (u32)nunits)), dim3(kBlock), 0, st, (const u64*)a,
                     (const u64*)b, (const u64*)c, (u64)n, (u32)nunits, (u64)add_a, (u64)add_b, (u64*)scratch, mtx_scan_array(scratch));
  hipLaunchKernelGGL(ibu_k_matrix_scan, dim3(1), dim3(kScanBlock), 0, st, mtx_scan_array(scratch), (u32)nunits);
  return hipGetLastError();
}
hipError_t launch_matrix_text_write(const LaunchCfg& cfg, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n, uint64_t add_a,
                                    uint64_t add_b, const void* scratch, char* text, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = mtx_units(n);
  hipLaunchKernelGGL(ibu_k_matrix_text_write, dim3(tiled_grid<ibu_k_matrix_text_write>(cfg, (u32)nunits)), dim3(kBlock), 0, st, (const u64*)a,
                     (const u64*)b, (const u64*)c, (u64)n, (u32)nunits, (u64)add_a, (u64)add_b, (const u64*)mtx_scan_array(scratch),
                     (uint8_t*)text);
  return hipGetLastError();
}

}  // namespace ibu
