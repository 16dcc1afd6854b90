// k_merge.hip — the stable two-way merge of sorted records (ibu_merge_sorted, ibu_merge_sorted_runs).  Design notes: kcommon.hpp,
// DESIGN.md §4 "Merge".  The semantics are this library's (the reference has no merge): include/ibu_hip.h.
//
// Order: the three words of a record in storage order, unsigned (rec_less of sort.hip).  Among equal records those of `a` come first:
//   a[i] lands at i + #{b <  a[i]}        b[j] lands at j + #{a <= b[j]}
// Three kernels:
//   ibu_k_merge_partition  one thread per output tile boundary d = t * kMergeTile: the number of a-records among the first d outputs,
//                          by the diagonal search on global memory, 8 bytes per boundary into the scratch.
//   ibu_k_merge<FAST, SRC> a wave owns output tile t = kMergeTile records = a[i0, i1) and b[j0, j1).  It stages both slices in its
//                          LDS share, ranks every a-record among the staged b-records (lower bound, binary search in LDS), marks
//                          the output slots e + rank as a's, and fills the slots in output order: slot p takes the next a-record
//                          where it is marked and the next b-record where it is not (ballot + mbcnt, no second search: the b-ranks
//                          are the complement of the a-ranks).  The records go back into the staging area in output order and leave
//                          as full 16-byte stores; the marks are the tile's source bytes as they stand.
//   ibu_k_merge_concat     leaves at once unless a merge kernel raised the `unsorted` word (below).
// Chosen over a per-lane sequential merge behind a second diagonal search: that form keeps two cursors and a 3-word compare per OUTPUT
// record with data-dependent LDS addresses (every lane on its own record: bank conflicts of any degree), this one searches per
// a-record only and moves records with stride-24 ds_read_b64 / ds_write_b64 at consecutive slots.
//
// Unsorted input.  Every index is clamped, so nothing is read or written outside the arrays whatever the records hold.  What
// unsorted input can break is consistency: boundary splits that are not monotone, or ranks inside a tile that are not.  Both are
// detected where they are computed (one compare each); the wave then raises `unsorted`, and ibu_k_merge_concat, which runs behind
// the merge in stream order, rewrites the output as a followed by b: a permutation of the input multiset, as the header promises.
#include "kcommon.hpp"
#include "kernels.h"

namespace ibu {

static constexpr int kMergeRounds = kMergeTile * 24 / 16 / kWave;     // 16-byte chunks of a tile per lane (6)
static constexpr int kMergePerLane = kMergeTile / kWave;              // records of a tile per lane (4)
// The wave's LDS share: the two slices (24 T bytes between them, each behind up to 8 bytes of phase, the second on a 16-byte
// boundary), reused for the tile in output order, and one mark byte per output slot.
static constexpr u32 kMergeStage = kMergeTile * 24 + 48;
static constexpr u32 kMergeWaveLds = kMergeStage + kMergeTile;
static_assert(kMergeTile % (16 * kWave / 4) == 0 && kMergeTile == 4 * kWave, "one u32 of marks per lane, whole rounds of chunks");
static_assert(kWavesPerBlock * kMergeWaveLds <= 65536, "the workgroup's LDS");

__device__ __forceinline__ bool merge_less(u64 b, u64 u, u64 x, u64 pb, u64 pu, u64 px) {   // (b,u,x) < (pb,pu,px): sort.hip rec_less
  return b != pb ? b < pb : (u != pu ? u < pu : x < px);
}
__device__ __forceinline__ u64 uniform64(u64 v) {      // a wave-uniform value into SGPRs (readfirstlane returns int: see WaveBuf)
  return ((u64)(u32)__builtin_amdgcn_readfirstlane((u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((u32)v);
}

// ---- partition -------------------------------------------------------------------------------------------------------------------
// split[t] = the number of a-records among the first d = min(t T, na + nb) outputs: the smallest i in [max(0, d - nb), min(d, na)]
// with a[i] > b[d - 1 - i].  Every index the loop reads is inside its array for any content (mid < min(d, na); d - 1 - mid in [0, nb)).
extern "C" __global__ void ibu_k_merge_partition(const u64* a, u64 na, const u64* b, u64 nb, u64 nbound, u64* __restrict__ split,
                                                 u64* __restrict__ unsorted) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) *unsorted = 0;
  if (t >= nbound) return;
  const u64 n = na + nb;
  u64 d = t * kMergeTile;
  d = d < n ? d : n;
  u64 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    const u64* pa = a + 3 * mid;
    const u64* pb = b + 3 * (d - 1 - mid);
    if (!merge_less(pb[0], pb[1], pb[2], pa[0], pa[1], pa[2])) lo = mid + 1;   // a[mid] <= b[d-1-mid]
    else hi = mid;
  }
  split[t] = lo;
}

// ---- merge -----------------------------------------------------------------------------------------------------------------------
// A slice of `len` records of one input as a wave stages it.  The slice starts 0 or 8 bytes behind a 16-byte boundary (`ph`); its
// whole 16-byte chunks ("interior") are loaded as such, and the 8 bytes in front of the first and behind the last of them, where
// there are any, as single words: nothing outside the slice is ever read, whatever the phase of the array and wherever it ends.
struct MergeSlice {
  const uint8_t* first;   // record 0 in global memory
  u32 bytes;              // 24 len
  u32 ph;                 // 8: a head word in front of the interior
  u32 nch;                // interior chunks, from first + ph
  u32 tailw;              // 8: a tail word behind the interior
  u32 lds;                // record 0 in the staging area; interior chunk k at lds + ph + 16 k
};
__device__ __forceinline__ MergeSlice merge_slice(const uint8_t* base, u64 first, u32 len, u32 lds_base /*a multiple of 16*/) {
  MergeSlice s;
  s.first = base + first * 24;
  s.bytes = len * 24;
  s.ph = len ? (u32)reinterpret_cast<uintptr_t>(s.first) & 8u : 0u;
  const u32 body = s.bytes - s.ph;
  s.nch = body >> 4;
  s.tailw = body & 8u;
  s.lds = lds_base + s.ph;
  return s;
}
struct MergeTile {        // wave-uniform
  MergeSlice A, B;
  u32 la, lb, dd;         // records of a, of b, of the tile
};
__device__ __forceinline__ MergeTile merge_tile(const uint8_t* a, const uint8_t* b, u64 d0, u64 i0, u32 la, u32 dd) {
  MergeTile m;
  m.la = la; m.lb = dd - la; m.dd = dd;
  m.A = merge_slice(a, i0, la, 0);
  m.B = merge_slice(b, d0 - i0, m.lb, (m.A.lds + m.A.bytes + 15u) & ~15u);
  return m;
}
struct MergeRegs {
  u32x4 v[kMergeRounds];
  u64 edge;               // lanes 0..3: head / tail word of a, of b
  u64 i0;                 // wave-uniform: the tile's first a-record, its a-records, and whether the splits had to be clamped
  u32 la;
  bool clamped;
};

// FAST: whole tiles, `out` (and `src`) 16-byte aligned — the tile leaves as full st16 stores; otherwise word and byte stores under a
// bound (the last, partial tile; an output of 8-byte phase).  SRC: the source bytes are wanted.
template <bool FAST, bool SRC>
__global__ void __launch_bounds__(kBlock, 4)
ibu_k_merge(const uint8_t* a, u64 na, const uint8_t* b, u64 nb, const u64* __restrict__ split, u64 t0, u32 ntiles, uint8_t* out,
            uint8_t* src, u64* unsorted) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kMergeWaveLds];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wib = threadIdx.x >> 6;
  uint8_t* const stage = lds + wib * kMergeWaveLds;
  uint8_t* const marks = stage + kMergeStage;          // marks[p]: 0 = output slot p takes an a-record, 1 = a b-record
  const u64 n = na + nb;
  bool bad = false;
  sweep_tiles<MergeRegs>(
      tile_range(ntiles, wib),
      [&](MergeRegs& g, u32 tv) {
        const u64 t = t0 + (u32)__builtin_amdgcn_readfirstlane(tv);
        const u64 d0 = t * kMergeTile;
        const u64 d1 = d0 + kMergeTile < n ? d0 + kMergeTile : n;
        const u32 dd = (u32)(d1 - d0);
        const u64 i0 = uniform64(split[t]), s1 = uniform64(split[t + 1]);
        // i1 in [i0, i0 + dd], not past na, and leaving b no more than it has: what sorted input gives anyway
        const u64 need = d1 > nb ? d1 - nb : 0;
        const u64 lo = i0 > need ? i0 : need, hi = i0 + dd < na ? i0 + dd : na;
        const u64 i1 = s1 < lo ? lo : (s1 > hi ? hi : s1);
        g.i0 = i0;
        g.la = (u32)(i1 - i0);
        g.clamped = i1 != s1;
        const MergeTile m = merge_tile(a, b, d0, i0, g.la, dd);
        const u32 last = m.A.nch + m.B.nch - 1;        // a tile has a record, and a slice with a record has an interior chunk
#pragma unroll
        for (int r = 0; r < kMergeRounds; ++r) {
          u32 c = lane + 64 * r;
          c = c < last ? c : last;                     // lanes past the last chunk re-read it
          const uint8_t* p = c < m.A.nch ? m.A.first + m.A.ph + 16 * (size_t)c : m.B.first + m.B.ph + 16 * (size_t)(c - m.A.nch);
          g.v[r] = ld16(p);
        }
        const bool of_b = lane & 2;                    // the four edge words, one lane each (an empty slice: any word of a)
        const uint8_t* sfirst = of_b ? m.B.first : m.A.first;
        const u32 sbytes = of_b ? m.B.bytes : m.A.bytes;
        const uint8_t* e = sbytes ? ((lane & 1) ? sfirst + sbytes - 8 : sfirst) : a;
        g.edge = __builtin_nontemporal_load(reinterpret_cast<const u64*>(e));
      },
      [&](const MergeRegs& g, u32 tv) {
        const u64 t = t0 + (u32)__builtin_amdgcn_readfirstlane(tv);
        const u64 d0 = t * kMergeTile;
        const u64 d1 = d0 + kMergeTile < n ? d0 + kMergeTile : n;
        const MergeTile m = merge_tile(a, b, d0, g.i0, g.la, (u32)(d1 - d0));
        bad = bad || g.clamped;
        // ---- registers -> LDS: the interior chunks, the edge words, the marks all "b"
        wave_lds_fence();
        const u32 ctot = m.A.nch + m.B.nch;
#pragma unroll
        for (int r = 0; r < kMergeRounds; ++r) {
          const u32 c = lane + 64 * r;
          const u32 off = c < m.A.nch ? m.A.lds + m.A.ph + 16 * c : m.B.lds + m.B.ph + 16 * (c - m.A.nch);
          if (c < ctot) *reinterpret_cast<u32x4*>(stage + off) = g.v[r];
        }
        {
          const bool of_b = lane & 2, tail = lane & 1;
          const u32 has = of_b ? (tail ? m.B.tailw : m.B.ph) : (tail ? m.A.tailw : m.A.ph);
          const u32 at = of_b ? m.B.lds + (tail ? m.B.bytes - 8 : 0) : m.A.lds + (tail ? m.A.bytes - 8 : 0);
          if (lane < 4 && has) *reinterpret_cast<u64*>(stage + at) = g.edge;
        }
        *reinterpret_cast<u32*>(marks + 4 * lane) = 0x01010101u;
        wave_lds_fence();
        // ---- a-record e ranks among the b-records: lower bound.  Output slot e + rank is an a-slot.
        u32 carry = 0;                                 // the rank of the a-record before this round's first
#pragma unroll
        for (int k = 0; k < kMergePerLane; ++k) {
          if (64u * k >= m.la) break;                  // wave-uniform
          const u32 e = lane + 64 * k;
          u32 rank = m.lb;
          if (e < m.la) {
            const u64* r = reinterpret_cast<const u64*>(stage + m.A.lds + 24 * e);
            const u64 x0 = r[0], x1 = r[1], x2 = r[2];
            u32 lo = 0, hi = m.lb;
            while (lo < hi) {
              const u32 mid = (lo + hi) >> 1;
              const u64* q = reinterpret_cast<const u64*>(stage + m.B.lds + 24 * mid);
              if (merge_less(q[0], q[1], q[2], x0, x1, x2)) lo = mid + 1;
              else hi = mid;
            }
            rank = lo;
            marks[e + rank] = 0;                       // e < la, rank <= lb: inside the tile
          }
          u32 prev = __shfl_up(rank, 1);
          if (lane == 0) prev = carry;
          bad = bad || rank < prev;                    // sorted input: ranks never fall
          carry = __shfl(rank, kWave - 1);
        }
        wave_lds_fence();
        // ---- output slot p takes a[#a-slots before p] or b[p - that]; all into registers, the staging area is reused for the output
        u64 rec[kMergePerLane][3];
        u32 before = 0;
        const u32 la1 = m.la ? m.la - 1 : 0, lb1 = m.lb ? m.lb - 1 : 0;
#pragma unroll
        for (int k = 0; k < kMergePerLane; ++k) {
          const u32 p = lane + 64 * k;
          const bool is_a = marks[p] == 0;
          const u64 mask = __ballot(is_a);
          const u32 ia = before + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
          before += (u32)__popcll(mask);
          u32 ib = p - ia;                             // sorted input and p < dd: below lb.  Clamped all the same.
          ib = ib < lb1 ? ib : lb1;
          const u32 off = is_a ? m.A.lds + 24 * (ia < la1 ? ia : la1) : m.B.lds + 24 * ib;
          const u64* r = reinterpret_cast<const u64*>(stage + off);
          rec[k][0] = r[0]; rec[k][1] = r[1]; rec[k][2] = r[2];
        }
        wave_lds_fence();
#pragma unroll
        for (int k = 0; k < kMergePerLane; ++k) {
          u64* w = reinterpret_cast<u64*>(stage + 24 * (lane + 64 * k));
          w[0] = rec[k][0]; w[1] = rec[k][1]; w[2] = rec[k][2];
        }
        wave_lds_fence();
        // ---- LDS -> global
        if constexpr (FAST) {
          uint8_t* q = out + d0 * 24 + 16 * lane;
#pragma unroll
          for (int r = 0; r < kMergeRounds; ++r) st16(q + 1024 * r, *reinterpret_cast<const u32x4*>(stage + 1024 * r + 16 * lane));
          if constexpr (SRC) {                         // 16 chunks of marks: the lanes behind them store them again
            const u32 c = lane & (kMergeTile / 16 - 1);
            st16(src + d0 + 16 * c, *reinterpret_cast<const u32x4*>(marks + 16 * c));
          }
        } else {
          u64* q = reinterpret_cast<u64*>(out) + d0 * 3;
#pragma unroll
          for (int r = 0; r < 3 * kMergePerLane; ++r) {
            const u32 w = lane + 64 * r;
            if (w < 3 * m.dd) q[w] = *reinterpret_cast<const u64*>(stage + 8 * w);
          }
          if constexpr (SRC) {
#pragma unroll
            for (int k = 0; k < kMergePerLane; ++k) {
              const u32 p = lane + 64 * k;
              if (p < m.dd) src[d0 + p] = marks[p];
            }
          }
        }
      });
  if (__ballot(bad) != 0 && lane == 0) *unsorted = 1;   // once per wave, behind the sweep (BadRows::flush)
}

// out = a followed by b, source bytes 0 then 1 — only where a merge kernel found its input unsorted.
extern "C" __global__ void ibu_k_merge_concat(const u64* a, u64 na, const u64* b, u64 nb, const u64* unsorted, u64* out, uint8_t* src) {
  if (*unsorted == 0) return;
  const u64 stride = (u64)gridDim.x * blockDim.x, first = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 wa = 3 * na, wb = 3 * nb;
  for (u64 w = first; w < wa; w += stride) out[w] = a[w];
  for (u64 w = first; w < wb; w += stride) out[wa + w] = b[w];
  if (src)
    for (u64 p = first; p < na + nb; p += stride) src[p] = p < na ? 0 : 1;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
size_t merge_scratch_bytes(size_t n) { return 8 * ((n + kMergeTile - 1) / kMergeTile + 2); }   // `unsorted`, one split per boundary

template <bool FAST, bool SRC>
static void launch_merge_tiles(const LaunchCfg& cfg, const void* a, size_t na, const void* b, size_t nb, const u64* split, u64 t0, u32 ntiles,
                               void* out, uint8_t* src, u64* unsorted, hipStream_t st) {
  static std::atomic<int> occ;
  hipLaunchKernelGGL((ibu_k_merge<FAST, SRC>), dim3(grid_for(ntiles, cfg.cus, resident_blocks<kBlock>(cfg, ibu_k_merge<FAST, SRC>, 0, &occ))),
                     dim3(kBlock), 0, st, (const uint8_t*)a, (u64)na, (const uint8_t*)b, (u64)nb, split, t0, ntiles, (uint8_t*)out, src, unsorted);
}

hipError_t launch_merge(const LaunchCfg& cfg, const void* a, size_t na, const void* b, size_t nb, void* out, uint8_t* src, void* scratch,
                        hipStream_t st) {
  (void)hipGetLastError();
  if (na == 0 || nb == 0) return hipErrorInvalidValue;           // a copy: the caller's
  const u64 n = (u64)na + nb, whole = n / kMergeTile, nbound = (n + kMergeTile - 1) / kMergeTile + 1;
  if (whole > 0xFFFFFFFFull) return hipErrorInvalidValue;        // n < 2^40
  u64* unsorted = reinterpret_cast<u64*>(scratch);
  u64* split = unsorted + 1;
  hipLaunchKernelGGL(ibu_k_merge_partition, dim3((u32)((nbound + 255) / 256)), dim3(256), 0, st, (const u64*)a, (u64)na, (const u64*)b, (u64)nb,
                     nbound, split, unsorted);
  const bool fast = aligned16(out) && (!src || aligned16(src));
  if (whole) {
    if (fast && src) launch_merge_tiles<true, true>(cfg, a, na, b, nb, split, 0, (u32)whole, out, src, unsorted, st);
    else if (fast) launch_merge_tiles<true, false>(cfg, a, na, b, nb, split, 0, (u32)whole, out, src, unsorted, st);
    else if (src) launch_merge_tiles<false, true>(cfg, a, na, b, nb, split, 0, (u32)whole, out, src, unsorted, st);
    else launch_merge_tiles<false, false>(cfg, a, na, b, nb, split, 0, (u32)whole, out, src, unsorted, st);
  }
  if (n % kMergeTile) {                                          // the partial tile
    if (src) launch_merge_tiles<false, true>(cfg, a, na, b, nb, split, whole, 1, out, src, unsorted, st);
    else launch_merge_tiles<false, false>(cfg, a, na, b, nb, split, whole, 1, out, src, unsorted, st);
  }
  hipLaunchKernelGGL(ibu_k_merge_concat, dim3(capped_grid(cfg, 3 * n, 256 * 8, 4)), dim3(256), 0, st, (const u64*)a, (u64)na, (const u64*)b,
                     (u64)nb, (const u64*)unsorted, (u64*)out, src);
  return hipGetLastError();
}

}  // namespace ibu
