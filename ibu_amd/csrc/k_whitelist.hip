// k_whitelist.hip — barcode correction against a whitelist: table build, correct, select (include/ibu_hip.h:
// ibu_whitelist_create, ibu_correct_barcodes, ibu_select_records), and what else probes the table: the abundance, resolve and
// the per-barcode labels (ibu_label_records).  Design notes: kcommon.hpp, DESIGN.md "Whitelist".
//
// The table: open addressing with linear probing over 64-bit keys, a power of two of slots, at most half of them
// taken, so a successful search looks at 1.5 slots on average and an unsuccessful one at 2.5 (linear probing at load
// 1/2: (1 + 1/(1-a))/2 and (1 + 1/(1-a)^2)/2); a slot's 128-byte line usually holds the whole probe sequence.  kEmpty
// (all ones) marks a free slot.  With 32 bases every 64-bit value is a legal code, all ones
// included: that one key never enters the table, the build reports it in a status word and every lookup gets it as a
// kernel argument (`has_ones`).  With fewer bases all ones has bits above 2*bc_len and is refused as a code anyway.
// Read-only after the build: any number of correct launches, on any streams, may probe it at once.
#include "kcommon.hpp"
#include "kernels.h"

namespace ibu {

static constexpr u64 kEmpty = ~0ull;

__device__ __forceinline__ u32 wl_slot(u64 key, u32 shift) {   // Fibonacci hashing: the top log2(slots) bits of key * phi
  return (u32)((key * 0x9E3779B97F4A7C15ull) >> shift);
}
__device__ __forceinline__ bool wl_lookup(const u64* __restrict__ table, u32 mask, u32 shift, u32 has_ones, u64 key) {
  if (key == kEmpty) return has_ones != 0;
  u32 s = wl_slot(key, shift) & mask;
  for (;;) {
    const u64 k = table[s];
    if (k == key) return true;
    if (k == kEmpty) return false;       // at most half the slots are taken: every probe sequence meets a free one
    s = (s + 1) & mask;
  }
}

// =============================================================================================
// build: one thread per code.  status[0] = lowest position of a code with bits at or above 2*bc_len (the caller sets
// it to all ones), status[1] = distinct codes, status[2] = 1 when the all-ones key is among them.
// =============================================================================================
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_whitelist_build(const u64* __restrict__ codes, u64 w, u64 high /*~mask2(bc_len)*/, u64* __restrict__ table, u32 mask, u32 shift,
                      u64* __restrict__ status) {
  const u64 stride = (u64)gridDim.x * kBlock;
  u64 first_bad = kEmpty;
  u32 fresh = 0;
  for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i < w; i += stride) {
    const u64 key = codes[i];
    if (key & high) { first_bad = i < first_bad ? i : first_bad; continue; }
    if (key == kEmpty) {
      if (atomicCAS(&status[2], 0ull, 1ull) == 0ull) ++fresh;
      continue;
    }
    u32 s = wl_slot(key, shift) & mask;
    for (;;) {
      const u64 old = atomicCAS(&table[s], kEmpty, key);
      if (old == kEmpty) { ++fresh; break; }
      if (old == key) break;             // a duplicate counts once
      s = (s + 1) & mask;
    }
  }
  first_bad = wave_reduce(first_bad, OpMin{});
  fresh = wave_reduce(fresh, OpAdd{});
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (first_bad != kEmpty) atomicMin(&status[0], first_bad);
    if (fresh) atomicAdd(&status[1], (u64)fresh);
  }
}

// =============================================================================================
// correct.  Classes: 0 exact, 1 corrected, 2 ambiguous, 3 unmatched (ibu_hip.h).
// =============================================================================================
struct WlArgs {
  const u64* table;
  u32 mask, shift, has_ones, bc_len;
  u32 search;      // max_mismatches
};

// Neighbour j of `low` (j in [0, 3*bc_len)): base j / 3 substituted by one of the three other bases.
__device__ __forceinline__ u64 wl_neighbour(u64 low, u32 j) {
  const u32 i = (j * 0xAAABu) >> 17;     // j / 3 for j < 2^15
  return low ^ ((u64)(j - 3 * i + 1) << (2 * i));
}

// One lane, one record: all 3*bc_len neighbours in turn (the tail kernel).
__device__ __forceinline__ u32 wl_search_lane(const WlArgs& a, u64 low, u64* fix) {
  u32 hits = 0;
  u64 cand = 0;
  for (u32 j = 0; j < 3 * a.bc_len; ++j) {
    const u64 nb = wl_neighbour(low, j);
    if (wl_lookup(a.table, a.mask, a.shift, a.has_ones, nb)) { if (hits++ == 0) cand = nb; }
  }
  *fix = cand;
  return hits == 1 ? 1u : hits ? 2u : 3u;
}

// The wave takes the barcodes of its missing lanes one after the other: lane L tests neighbours L and L + 64 (3*bc_len
// is at most 96), the ballots give the number of whitelisted neighbours and, where it is one, which.  A miss costs the
// wave two probe rounds instead of a lane 96 of them with the other 63 lanes waiting.  `miss` is the lane's own flag;
// returns the lane's class (3 where it did not miss is never read) and its corrected barcode.
__device__ __forceinline__ u32 wl_search_wave(const WlArgs& a, bool miss, u64 low, u64* fix, u32 lane) {
  u64 todo = __ballot(miss);
  u32 cls = 3;
  u64 cand = 0;
  const u32 nn = 3 * a.bc_len;
  while (todo) {                                   // wave-uniform
    const u32 src = (u32)__builtin_ctzll(todo);
    todo &= todo - 1;
    const u64 bc = ((u64)(u32)__builtin_amdgcn_readlane((u32)(low >> 32), src) << 32) | (u64)(u32)__builtin_amdgcn_readlane((u32)low, src);
    const bool h0 = lane < nn && wl_lookup(a.table, a.mask, a.shift, a.has_ones, wl_neighbour(bc, lane));
    const u64 b0 = __ballot(h0);
    u64 b1 = 0;
    if (nn > 64) {                                 // wave-uniform
      const bool h1 = lane + 64 < nn && wl_lookup(a.table, a.mask, a.shift, a.has_ones, wl_neighbour(bc, lane + 64));
      b1 = __ballot(h1);
    }
    const u32 hits = (u32)__builtin_popcountll(b0) + (u32)__builtin_popcountll(b1);
    const u32 j = b0 ? (u32)__builtin_ctzll(b0) : 64u + (u32)__builtin_ctzll(b1 | (1ull << 63));
    if (lane == src) {
      cls = hits == 1 ? 1u : hits ? 2u : 3u;
      cand = wl_neighbour(bc, j);
    }
  }
  *fix = cand;
  return cls;
}

// The totals of ibu_k_correct and its tail, on the path they had before block_accumulate (kcommon.hpp) took over everywhere else:
// lane counters -> wave (shuffles) -> workgroup (LDS) -> one atomic per class and workgroup into slot blockIdx % kReduceSlots of
// `acc` (kReduceSlots x 4 u64, folded by ibu_k_correct_fold).  Kept because ibu_k_correct measured 0.5 % slower over 1e9 records
// with block_accumulate behind its sweep, with no totals asked for: the sweep's register allocation moves with what follows it
// (profiles/README.md r22_a).
__device__ __forceinline__ void wl_flush_totals(u32 cnt[4], u64* acc, u32 (*part)[4]) {
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int c = 0; c < 4; ++c) cnt[c] += __shfl_xor(cnt[c], m);
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) part[wib][c] = cnt[c];
  __syncthreads();
  if (threadIdx.x < 4) {
    u64 v = 0;
    for (u32 k = 0; k < blockDim.x / kWave; ++k) v += part[k][threadIdx.x];
    if (v) atomicAdd(&acc[4 * (blockIdx.x & (kReduceSlots - 1)) + threadIdx.x], v);
  }
}

struct CorrectArgs { WlArgs wl; u64* acc; };     // acc: nullable, uniform over the grid

// Tiled (kcommon.hpp: sweep_records).  Nothing of a record is stored but the 8 barcode bytes of a corrected one.  Misses: the
// wave-cooperative neighbour search (the form in which every lane searched its own record measured 2-4.7x slower:
// profiles/README.md r06_a).
extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_correct(uint8_t* __restrict__ recs, u32 ntiles, uint8_t* __restrict__ cls_out, const CorrectArgs ca) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kTileBytes];
  __shared__ u32 part[kWavesPerBlock][4];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  uint8_t* tile = lds + wib * kTileBytes;
  const WlArgs& a = ca.wl;
  const u64 m = mask2(a.bc_len);
  u32 cnt[4] = {0, 0, 0, 0};
  sweep_records(recs, ntiles, tile, lane, wib, [&](u32 t) {
    u64 bc[2], fix[2];
    u32 c[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bc[h] = rec_word(tile, lane, h);
      c[h] = wl_lookup(a.table, a.mask, a.shift, a.has_ones, bc[h] & m) ? 0u : 3u;
      fix[h] = 0;
    }
    if (a.search) {                                  // wave-uniform
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32 s = wl_search_wave(a, c[h] != 0, bc[h] & m, &fix[h], lane);
        if (c[h] != 0) c[h] = s;
      }
    }
    u64* r = reinterpret_cast<u64*>(recs + (size_t)t * kTileBytes) + 6 * lane;   // records 2L, 2L+1: words 6L and 6L+3
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (c[h] == 1) r[3 * h] = (bc[h] & ~m) | fix[h];
      cnt[0] += c[h] == 0; cnt[1] += c[h] == 1; cnt[2] += c[h] == 2; cnt[3] += c[h] == 3;
    }
    if (cls_out) store_class_pair(cls_out, t, lane, c[0], c[1]);   // wave-uniform
  });
  if (ca.acc) wl_flush_totals(cnt, ca.acc, part);    // uniform over the grid
}

// One thread per record: the rows peeled off the front of an 8- but not 16-byte aligned array and the n % 128 rest.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_correct_tail(u64* __restrict__ recs, u64 row0, u64 n, uint8_t* __restrict__ cls_out, const CorrectArgs ca) {
  __shared__ u32 part[kWavesPerBlock][4];
  const WlArgs& a = ca.wl;
  const u64 i = row0 + (u64)blockIdx.x * kBlock + threadIdx.x;
  u32 cnt[4] = {0, 0, 0, 0};
  if (i < n) {
    const u64 m = mask2(a.bc_len), bc = recs[3 * i];
    u32 c = wl_lookup(a.table, a.mask, a.shift, a.has_ones, bc & m) ? 0u : 3u;
    if (c && a.search) {
      u64 fix;
      c = wl_search_lane(a, bc & m, &fix);
      if (c == 1) recs[3 * i] = (bc & ~m) | fix;
    }
    if (cls_out) cls_out[i] = (uint8_t)c;
    cnt[0] = c == 0; cnt[1] = c == 1; cnt[2] = c == 2; cnt[3] = c == 3;
  }
  if (ca.acc) wl_flush_totals(cnt, ca.acc, part);
}

// slots -> slot 0: one wave, lane = slot
extern "C" __global__ void ibu_k_correct_fold(u64* acc) {
  const u32 lane = threadIdx.x;
  u64 v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = acc[4 * lane + c];
  wave_reduce(v, OpAdd{});
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = v[c];
}

// =============================================================================================
// select: stable compaction by class.  A UNIT is 2048 consecutive records and belongs to one wave, so nothing here
// needs a workgroup barrier: count (kept records per unit) -> scan (exclusive, in place, total in front) -> scatter
// (a unit's kept records, in input order, from its offset on).
// =============================================================================================
static constexpr u32 kSelUnit = 2048, kSelRounds = kSelUnit / kWave;

__device__ __forceinline__ bool sel_keep(const uint8_t* __restrict__ cls, u64 i, u64 n, u32 keep_mask) {
  const u32 c = i < n ? cls[i] : 255u;
  return c < 8u && ((keep_mask >> c) & 1u);
}

// units[0] = total (after the scan); units[1 + u] = kept records of unit u, then their exclusive prefix sum
extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_select_count(const uint8_t* __restrict__ cls, u64 n, u32 nunits, u32 keep_mask, u64* __restrict__ units) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    u32 k = 0;
#pragma unroll 8
    for (u32 r = 0; r < kSelRounds; ++r) k += sel_keep(cls, (u64)u * kSelUnit + r * kWave + lane, n, keep_mask);
    k = wave_reduce(k, OpAdd{});
    if (lane == 0) units[1 + u] = k;
  }
}

// One workgroup of kScanBlock threads: kcommon.hpp, scan_units_in_place (shared with the matrix export, k_matrix.hip).
extern "C" __global__ void __launch_bounds__(kScanBlock)
ibu_k_select_scan(u64* __restrict__ units, u32 nunits) {
  scan_units_in_place(units, nunits);
}

extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_select_scatter(const u64* __restrict__ recs, const uint8_t* __restrict__ cls, u64 n, u32 nunits, u32 keep_mask,
                     const u64* __restrict__ units, u64* __restrict__ out) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    u64 pos = units[1 + u];
#pragma unroll 4
    for (u32 r = 0; r < kSelRounds; ++r) {
      const u64 i = (u64)u * kSelUnit + r * kWave + lane;
      const bool keep = sel_keep(cls, i, n, keep_mask);
      const u64 b = __ballot(keep);
      if (keep) {
        const u64* s = recs + 3 * i;
        u64* d = out + 3 * (pos + (u32)__builtin_popcountll(b & below));
        const u64 x = __builtin_nontemporal_load(s), y = __builtin_nontemporal_load(s + 1), z = __builtin_nontemporal_load(s + 2);
        __builtin_nontemporal_store(x, d); __builtin_nontemporal_store(y, d + 1); __builtin_nontemporal_store(z, d + 2);
      }
      pos += (u32)__builtin_popcountll(b);
    }
  }
}

// =============================================================================================
// abundance and resolve (ibu_abundance_add, ibu_abundance_counts, ibu_resolve_barcodes).  An abundance is one u64 counter
// per table slot and one more, at index `slots`, for the all-ones key that never enters the table.  add counts the records
// whose barcode is in the whitelist; resolve gives an ambiguous record (class 2) to the candidate that holds at least
// num / den of its candidates' reads.
// The adds are scattered 8-byte integer atomics: one per counted record on input in read order.  Their rate on this chip
// is not measured anywhere (the guides price float atomics, as bytes of well-shaped rows): profiles/README.md r15_a.
// =============================================================================================
static constexpr u64 kNoSlot = ~0ull;

// wl_lookup that says where: the key's slot, `slots` for the all-ones key, kNoSlot for a key that is not in the whitelist.
__device__ __forceinline__ u64 wl_lookup_slot(const u64* __restrict__ table, u32 mask, u32 shift, u32 has_ones, u64 key) {
  if (key == kEmpty) return has_ones ? (u64)mask + 1 : kNoSlot;
  u32 s = wl_slot(key, shift) & mask;
  for (;;) {
    const u64 k = table[s];
    if (k == key) return s;
    if (k == kEmpty) return kNoSlot;
    s = (s + 1) & mask;
  }
}
__device__ __forceinline__ bool ab_counted(const uint8_t* __restrict__ cls, u64 i, u32 class_mask) {
  if (!cls) return true;
  const u32 c = cls[i];
  return c < 8u && ((class_mask >> c) & 1u);
}
__device__ __forceinline__ void ab_add(u64* __restrict__ counters, u64 slot, u64 v) {   // no value comes back: a no-return atomic
  (void)__hip_atomic_fetch_add(counters + slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct AbundanceArgs { WlArgs wl; u32 class_mask; u64* counters; };

// Tiled (kcommon.hpp: sweep_records).  Grouped input (sorted records, a few hot barcodes) would put the 128 adds of a tile on one
// address, so runs of equal slot inside the tile are merged first (kcommon.hpp: next_head; the record before a lane's first one
// comes by shuffle), and a head whose slot counts issues one atomic with the run's length.
extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_abundance_add(const uint8_t* __restrict__ recs, u32 ntiles, const uint8_t* __restrict__ cls, const AbundanceArgs aa) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kTileBytes];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  uint8_t* tile = lds + wib * kTileBytes;
  const WlArgs& a = aa.wl;
  const u64 m = mask2(a.bc_len);
  sweep_records(recs, ntiles, tile, lane, wib, [&](u32 t) {
    u64 s[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u64 bc = rec_word(tile, lane, h);
      s[h] = ab_counted(cls, (u64)t * kTileRecs + 2 * lane + h, aa.class_mask) ? wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, bc & m)
                                                                                : kNoSlot;
    }
    const u64 prev = shfl_up64(s[1], 1);
    const bool head0 = lane == 0 || s[0] != prev, head1 = s[1] != s[0];
    const u32 next = next_head(__ballot(head0), __ballot(head1), lane, kTileRecs);
    if (head0 && s[0] != kNoSlot) ab_add(aa.counters, s[0], head1 ? 1u : next - 2 * lane);
    if (head1 && s[1] != kNoSlot) ab_add(aa.counters, s[1], next - (2 * lane + 1));
  });
}

// One thread per record: the peeled head and the n % 128 rest.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_abundance_add_tail(const u64* __restrict__ recs, u64 row0, u64 n, const uint8_t* __restrict__ cls, const AbundanceArgs aa) {
  const WlArgs& a = aa.wl;
  const u64 i = row0 + (u64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || !ab_counted(cls, i, aa.class_mask)) return;
  const u64 s = wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, recs[3 * i] & mask2(a.bc_len));
  if (s != kNoSlot) ab_add(aa.counters, s, 1);
}

// out[j] = the counter of codes[j]; 0 for a code that is not in the whitelist or has bits at or above 2*bc_len.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_abundance_counts(const u64* __restrict__ codes, u64 k, const WlArgs a, const u64* __restrict__ counters, u64* __restrict__ out) {
  const u64 stride = (u64)gridDim.x * kBlock, m = mask2(a.bc_len);
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < k; j += stride) {
    const u64 key = codes[j];
    const u64 s = (key & ~m) ? kNoSlot : wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, key);
    out[j] = s != kNoSlot ? counters[s] : 0;
  }
}

// One round of resolve: every lane brings at most one class-2 record (`has`, row `idx`) and gathers its barcode; the wave
// takes them one after the other, as wl_search_wave does: lane L probes neighbours L and L + 64 and loads their counters,
// the reductions give total and best, the ballots of "hit and count == best" name the winner (one candidate only: best > 0
// and best / total >= num / den > 1/2), and the record's own lane writes the 8 barcode bytes and the class byte.
// cnt: examined, resolved, below the share, unseen.
__device__ __forceinline__ void resolve_round(const WlArgs& a, const u64* __restrict__ counters, u64 num, u64 den, u64* recs, uint8_t* cls,
                                              bool has, u64 idx, u32 lane, u32 cnt[4]) {
  const u64 m = mask2(a.bc_len);
  const u64 bc = has ? recs[3 * idx] : 0;
  const u32 nn = 3 * a.bc_len;
  u64 todo = __ballot(has);
  while (todo) {                                     // wave-uniform
    const u32 src = (u32)__builtin_ctzll(todo);
    todo &= todo - 1;
    const u64 low = (((u64)(u32)__builtin_amdgcn_readlane((u32)(bc >> 32), src) << 32) | (u64)(u32)__builtin_amdgcn_readlane((u32)bc, src)) & m;
    u64 c0 = 0, c1 = 0;
    bool hit0 = false, hit1 = false;
    if (lane < nn) {
      const u64 s = wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, wl_neighbour(low, lane));
      hit0 = s != kNoSlot;
      if (hit0) c0 = counters[s];
    }
    if (lane + 64 < nn) {
      const u64 s = wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, wl_neighbour(low, lane + 64));
      hit1 = s != kNoSlot;
      if (hit1) c1 = counters[s];
    }
    const u64 total = wave_reduce(c0 + c1, OpAdd{});
    const u64 best = wave_reduce(c0 > c1 ? c0 : c1, OpMax{});
    const bool win = best > 0 && best * den >= num * total;   // counters sum to at most 2^40, den < 2^24: no overflow
    const u64 b0 = __ballot(hit0 && c0 == best), b1 = __ballot(hit1 && c1 == best);
    const u32 j = b0 ? (u32)__builtin_ctzll(b0) : 64u + (u32)__builtin_ctzll(b1 | (1ull << 63));
    if (lane == src) {
      ++cnt[0];
      if (win) {
        recs[3 * idx] = (bc & ~m) | wl_neighbour(low, j);
        cls[idx] = 4;                                // IBU_BARCODE_RESOLVED
        ++cnt[1];
      } else if (total) ++cnt[2];
      else ++cnt[3];
    }
  }
}

// The four-bit mask of the bytes of w that equal 2 (bit k: byte k).
__device__ __forceinline__ u32 bytes_eq2(u32 w) {
  const u32 x = w ^ 0x02020202u;
  const u32 z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every byte of x that is zero, exactly
  return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;                          // bits 0, 8, 16, 24 -> bits 21..24 (no two terms meet)
}

// Driven by the class bytes (16-byte aligned here): a UNIT is 1024 of them, one 16-byte load per lane.  A record is touched
// only where its class is 2.
static constexpr u32 kResolveUnit = 16 * kWave;
extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_resolve(u64* recs, uint8_t* cls, u32 nunits, const WlArgs a, const u64* __restrict__ counters, u64 num, u64 den, u64* __restrict__ acc) {
  __shared__ u64 accl[kWavesPerBlock * 4];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  u32 cnt[4] = {0, 0, 0, 0};
  const TileRange tr = tile_range(nunits, wib);
  for (u32 t = tr.t; t < tr.end; t += tr.stride) {   // wave-uniform
    const u64 base = (u64)t * kResolveUnit + 16 * lane;
    const u32x4 v = *reinterpret_cast<const u32x4*>(cls + base);
    u32 m16 = bytes_eq2(v.x) | (bytes_eq2(v.y) << 4) | (bytes_eq2(v.z) << 8) | (bytes_eq2(v.w) << 12);
    while (__ballot(m16 != 0)) {                     // wave-uniform: every lane's next class-2 record
      const bool has = m16 != 0;
      resolve_round(a, counters, num, den, recs, cls, has, base + (has ? (u32)__builtin_ctz(m16) : 0u), lane, cnt);
      m16 &= m16 - 1;
    }
  }
  u64 t[4] = {cnt[0], cnt[1], cnt[2], cnt[3]};
  if (acc) block_accumulate(t, acc, accl);           // uniform over the grid
}

// One class byte per lane: the bytes in front of the first 16-byte boundary of the class array and the rest behind the last unit.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_resolve_tail(u64* recs, uint8_t* cls, u64 row0, u64 row1, const WlArgs a, const u64* __restrict__ counters, u64 num, u64 den,
                   u64* __restrict__ acc) {
  __shared__ u64 accl[kWavesPerBlock * 4];
  const u64 i = row0 + (u64)blockIdx.x * kBlock + threadIdx.x;
  u32 cnt[4] = {0, 0, 0, 0};
  resolve_round(a, counters, num, den, recs, cls, i < row1 && cls[i] == 2, i, threadIdx.x & (kWave - 1), cnt);
  u64 t[4] = {cnt[0], cnt[1], cnt[2], cnt[3]};
  if (acc) block_accumulate(t, acc, accl);
}

// =============================================================================================
// labels (ibu_labels_set, ibu_labels_get, ibu_label_records).  A label table is the abundance's shape with one BYTE per table
// slot and one more, at index `slots`, for the all-ones key.  Labelling is one probe and one gathered byte per record; a record
// whose barcode is not an entry has bin kLabelMissing.  The histogram (257 bins) costs no global atomic per record: runs of equal
// bin inside a tile are merged as ibu_k_abundance_add merges runs of equal slot, a run's length goes into the workgroup's LDS
// histogram, and the workgroup flushes its non-zero bins once, when its sweep is over, into slot blockIdx % kReduceSlots of `acc`
// (kReduceSlots x kLabelBins u64, folded by ibu_k_label_fold).  The LDS bins are u64: no sweep length can overflow them.
// =============================================================================================
static constexpr u32 kLabelMissing = 256, kLabelBins = 257;

struct LabelArgs {
  WlArgs wl;
  const uint8_t* labels;
  u32 match_mode;   // 0: class = label, or `missing` where not found; 1: 0 label == match, 1 another label, 2 not found
  u32 match, missing;
  u64* acc;         // the histogram slots; nullable, uniform over the grid
};
__device__ __forceinline__ u32 label_bin(const LabelArgs& l, u64 low) {
  const WlArgs& a = l.wl;
  const u64 s = wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, low);
  return s != kNoSlot ? (u32)l.labels[s] : kLabelMissing;
}
__device__ __forceinline__ u32 label_class(const LabelArgs& l, u32 bin) {
  if (l.match_mode) return bin == kLabelMissing ? 2u : bin == l.match ? 0u : 1u;
  return bin == kLabelMissing ? l.missing : bin;
}
__device__ __forceinline__ void label_hist_add(u64* hist, u32 bin, u32 v) {   // no value comes back: a no-return LDS atomic
  (void)__hip_atomic_fetch_add(hist + bin, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void label_hist_clear(u64* hist) {   // every thread of the workgroup calls
  for (u32 b = threadIdx.x; b < kLabelBins; b += blockDim.x) hist[b] = 0;
  __syncthreads();
}
__device__ __forceinline__ void label_hist_flush(const u64* hist, u64* __restrict__ acc) {   // every thread of the workgroup calls
  __syncthreads();
  u64* slot = acc + (size_t)kLabelBins * (blockIdx.x & (kReduceSlots - 1));
  for (u32 b = threadIdx.x; b < kLabelBins; b += blockDim.x) {
    const u64 v = hist[b];
    if (v) atomicAdd(&slot[b], v);
  }
}

// Tiled (kcommon.hpp: sweep_records).  HIST: the call asked for the histogram (l.acc != NULL); runs of equal bin inside the tile are
// merged as ibu_k_abundance_add merges runs of equal slot.
template <bool HIST>
__global__ void __launch_bounds__(kBlock, 8)
ibu_k_label(const uint8_t* __restrict__ recs, u32 ntiles, uint8_t* __restrict__ cls_out, const LabelArgs l) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kTileBytes];
  __shared__ u64 hist[HIST ? kLabelBins : 1];
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  uint8_t* tile = lds + wib * kTileBytes;
  const u64 m = mask2(l.wl.bc_len);
  if constexpr (HIST) label_hist_clear(hist);
  sweep_records(recs, ntiles, tile, lane, wib, [&](u32 t) {
    u32 b[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) b[h] = label_bin(l, rec_word(tile, lane, h) & m);
    if (cls_out) store_class_pair(cls_out, t, lane, label_class(l, b[0]), label_class(l, b[1]));   // wave-uniform
    if constexpr (HIST) {
      const u32 prev = __shfl_up(b[1], 1);
      const bool head0 = lane == 0 || b[0] != prev, head1 = b[1] != b[0];
      const u32 next = next_head(__ballot(head0), __ballot(head1), lane, kTileRecs);
      if (head0) label_hist_add(hist, b[0], head1 ? 1u : next - 2 * lane);
      if (head1) label_hist_add(hist, b[1], next - (2 * lane + 1));
    }
  });
  if constexpr (HIST) label_hist_flush(hist, l.acc);
}

// One thread per record: the peeled head and the n % 128 rest.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_label_tail(const u64* __restrict__ recs, u64 row0, u64 n, uint8_t* __restrict__ cls_out, const LabelArgs l) {
  __shared__ u64 hist[kLabelBins];
  const u64 i = row0 + (u64)blockIdx.x * kBlock + threadIdx.x;
  if (l.acc) label_hist_clear(hist);
  if (i < n) {
    const u32 b = label_bin(l, recs[3 * i] & mask2(l.wl.bc_len));
    if (cls_out) cls_out[i] = (uint8_t)label_class(l, b);
    if (l.acc) label_hist_add(hist, b, 1);
  }
  if (l.acc) label_hist_flush(hist, l.acc);
}

// slots -> slot 0: thread b sums bin b of every slot (it alone reads and writes bin b of slot 0)
extern "C" __global__ void ibu_k_label_fold(u64* acc) {
  const u32 b = threadIdx.x;
  if (b >= kLabelBins) return;
  u64 v = 0;
  for (u32 s = 0; s < (u32)kReduceSlots; ++s) v += acc[(size_t)kLabelBins * s + b];
  acc[b] = v;
}

// The label of codes[j] becomes vals[j] (byte stores only); a code that is not in the whitelist or has bits at or above 2*bc_len
// is skipped and, with skipped != NULL (uniform over the grid), counted there.  No thread leaves the loop by `return`: all of them
// reach block_accumulate's barrier.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_labels_set(const u64* __restrict__ codes, const uint8_t* __restrict__ vals, u64 k, const WlArgs a, uint8_t* __restrict__ labels,
                 u64* __restrict__ skipped) {
  __shared__ u64 accl[kWavesPerBlock];
  const u64 stride = (u64)gridDim.x * kBlock, m = mask2(a.bc_len);
  u32 miss = 0;
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < k; j += stride) {
    const u64 key = codes[j];
    const u64 s = (key & ~m) ? kNoSlot : wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, key);
    if (s != kNoSlot) labels[s] = vals[j];
    else ++miss;
  }
  u64 t[1] = {miss};
  if (skipped) block_accumulate(t, skipped, accl);
}

// out[j] = the label of codes[j]; `missing` for a code that is not in the whitelist or has bits at or above 2*bc_len.
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_labels_get(const u64* __restrict__ codes, u64 k, const WlArgs a, const uint8_t* __restrict__ labels, u32 missing, uint8_t* __restrict__ out) {
  const u64 stride = (u64)gridDim.x * kBlock, m = mask2(a.bc_len);
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < k; j += stride) {
    const u64 key = codes[j];
    const u64 s = (key & ~m) ? kNoSlot : wl_lookup_slot(a.table, a.mask, a.shift, a.has_ones, key);
    out[j] = s != kNoSlot ? labels[s] : (uint8_t)missing;
  }
}

// =============================================================================================
// Launchers
// =============================================================================================
size_t whitelist_slots(size_t w) {   // a power of two, at least 2 w (load factor at most 1/2) and at least 1024
  size_t s = 1024;
  while (s < 2 * w) s <<= 1;
  return s;
}
static inline u32 log2_of(size_t pow2) { u32 l = 0; while (((size_t)1 << l) < pow2) ++l; return l; }

hipError_t launch_whitelist_build(const LaunchCfg& cfg, const uint64_t* codes, size_t w, uint32_t bc_len, uint64_t* table, size_t slots,
                                  uint64_t* status, hipStream_t st) {
  (void)hipGetLastError();
  if (w == 0) return hipSuccess;
  if (slots < 2 * w || (slots & (slots - 1)) || slots > (1ull << 32)) return hipErrorInvalidValue;
  u64 blocks = (w + kBlock - 1) / kBlock;
  static std::atomic<int> occ;
  const u64 cap = (u64)cfg.cus * resident_blocks<kBlock>(cfg, ibu_k_whitelist_build, 0, &occ);
  if (blocks > cap) blocks = cap;
  const u64 high = bc_len >= 32 ? 0ull : ~((1ull << (2 * bc_len)) - 1);   // the bits no code may have
  hipLaunchKernelGGL(ibu_k_whitelist_build, dim3((u32)blocks), dim3(kBlock), 0, st, (const u64*)codes, (u64)w, high,
                     (u64*)table, (u32)(slots - 1), 64u - log2_of(slots), (u64*)status);
  return hipGetLastError();
}

static inline WlArgs wl_args(const WhitelistTable& wl, uint32_t search) {
  WlArgs a;
  a.table = (const u64*)wl.table; a.mask = (u32)(wl.slots - 1); a.shift = 64u - log2_of(wl.slots); a.has_ones = wl.has_ones ? 1u : 0u;
  a.bc_len = wl.bc_len; a.search = search;
  return a;
}
hipError_t launch_correct(const LaunchCfg& cfg, const WhitelistTable& wl, void* recs, size_t n, uint32_t max_mismatches, uint8_t* d_class,
                          uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  if (n / kTileRecs > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const hipError_t e = zero_totals(acc, kCorrectAccBytes / sizeof(u64), st);
  if (e != hipSuccess || n == 0) return e;
  launch_record_pass<ibu_k_correct, ibu_k_correct_tail>(cfg, recs, n, d_class, CorrectArgs{wl_args(wl, max_mismatches), (u64*)acc}, st);
  if (acc) hipLaunchKernelGGL(ibu_k_correct_fold, dim3(1), dim3(kReduceSlots), 0, st, (u64*)acc);
  return hipGetLastError();
}

hipError_t launch_abundance_add(const LaunchCfg& cfg, const WhitelistTable& wl, const void* recs, const uint8_t* d_class, size_t n,
                                uint32_t class_mask, uint64_t* counters, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  if (n / kTileRecs > 0xFFFFFFFFull) return hipErrorInvalidValue;
  launch_record_pass<ibu_k_abundance_add, ibu_k_abundance_add_tail>(cfg, recs, n, d_class, AbundanceArgs{wl_args(wl, 0), class_mask, (u64*)counters},
                                                                    st);
  return hipGetLastError();
}
hipError_t launch_abundance_counts(const LaunchCfg& cfg, const WhitelistTable& wl, const uint64_t* counters, const uint64_t* codes, size_t k,
                                   uint64_t* out, hipStream_t st) {
  (void)hipGetLastError();
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(ibu_k_abundance_counts, dim3(capped_grid(cfg, k, kBlock)), dim3(kBlock), 0, st, (const u64*)codes, (u64)k, wl_args(wl, 0),
                     (const u64*)counters, (u64*)out);
  return hipGetLastError();
}
hipError_t launch_resolve(const LaunchCfg& cfg, const WhitelistTable& wl, const uint64_t* counters, void* recs, size_t n, uint64_t num,
                          uint64_t den, uint8_t* d_class, uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  const hipError_t e = zero_totals(acc, 4, st);
  if (e != hipSuccess || n == 0) return e;
  const WlArgs a = wl_args(wl, 1);
  const Span sp[1] = {{d_class, 1}};   // the split is the class bytes': those in front of the first 16-byte boundary are the head
  launch_rows(cfg, sp, 1, n, kResolveUnit,
      [&](u64 row0, u64 row1) {
        hipLaunchKernelGGL(ibu_k_resolve_tail, dim3(tail_grid(row1 - row0)), dim3(kBlock), 0, st, (u64*)recs, d_class, row0, row1, a,
                           (const u64*)counters, (u64)num, (u64)den, (u64*)acc);
      },
      [&](size_t head, u32 nunits) {   // n < 2^40: nunits below 2^30
        hipLaunchKernelGGL(ibu_k_resolve, dim3(tiled_grid<ibu_k_resolve>(cfg, nunits)), dim3(kBlock), 0, st, adv((u64*)recs, 24 * head),
                           d_class + head, nunits, a, (const u64*)counters, (u64)num, (u64)den, (u64*)acc);
      });
  return hipGetLastError();
}

static_assert(kLabelAccBytes == (size_t)kReduceSlots * kLabelBins * sizeof(u64), "kernels.h sizes the histogram slots");
hipError_t launch_labels_set(const LaunchCfg& cfg, const WhitelistTable& wl, uint8_t* labels, const uint64_t* codes, const uint8_t* vals, size_t k,
                             uint64_t* skipped, hipStream_t st) {
  (void)hipGetLastError();
  const hipError_t e = zero_totals(skipped, 1, st);
  if (e != hipSuccess || k == 0) return e;
  hipLaunchKernelGGL(ibu_k_labels_set, dim3(capped_grid(cfg, k, kBlock)), dim3(kBlock), 0, st, (const u64*)codes, vals, (u64)k, wl_args(wl, 0),
                     labels, (u64*)skipped);
  return hipGetLastError();
}
hipError_t launch_labels_get(const LaunchCfg& cfg, const WhitelistTable& wl, const uint8_t* labels, const uint64_t* codes, size_t k,
                             uint32_t missing, uint8_t* out, hipStream_t st) {
  (void)hipGetLastError();
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(ibu_k_labels_get, dim3(capped_grid(cfg, k, kBlock)), dim3(kBlock), 0, st, (const u64*)codes, (u64)k, wl_args(wl, 0), labels,
                     missing, out);
  return hipGetLastError();
}
hipError_t launch_label_records(const LaunchCfg& cfg, const WhitelistTable& wl, const uint8_t* labels, const void* recs, size_t n, bool match_mode,
                                uint32_t match, uint32_t missing_class, uint8_t* d_class, uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0 || (!d_class && !acc)) return hipSuccess;
  if (n / kTileRecs > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const LabelArgs l{wl_args(wl, 0), labels, match_mode ? 1u : 0u, match, missing_class, (u64*)acc};
  if (acc) launch_record_pass<ibu_k_label<true>, ibu_k_label_tail>(cfg, recs, n, d_class, l, st);
  else launch_record_pass<ibu_k_label<false>, ibu_k_label_tail>(cfg, recs, n, d_class, l, st);
  return hipGetLastError();
}
hipError_t launch_label_fold(uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(ibu_k_label_fold, dim3(1), dim3(320), 0, st, (u64*)acc);   // five waves: a thread per bin
  return hipGetLastError();
}

size_t select_scratch_bytes(size_t n) { return 8 * (1 + (n + kSelUnit - 1) / kSelUnit); }
hipError_t launch_select_count(const LaunchCfg& cfg, const uint8_t* d_class, size_t n, uint32_t keep_mask, void* scratch, size_t scratch_bytes,
                               hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = (n + kSelUnit - 1) / kSelUnit;
  if (nunits > 0xFFFFFFFFull || scratch_bytes < select_scratch_bytes(n)) return hipErrorInvalidValue;
  static std::atomic<int> occ;
  hipLaunchKernelGGL(ibu_k_select_count, dim3(grid_for((u32)nunits, cfg.cus, resident_blocks<kBlock>(cfg, ibu_k_select_count, 0, &occ))),
                     dim3(kBlock), 0, st, d_class, (u64)n, (u32)nunits, keep_mask, (u64*)scratch);
  hipLaunchKernelGGL(ibu_k_select_scan, dim3(1), dim3(kScanBlock), 0, st, (u64*)scratch, (u32)nunits);
  return hipGetLastError();
}
hipError_t launch_select_scatter(const LaunchCfg& cfg, const void* recs, const uint8_t* d_class, size_t n, uint32_t keep_mask,
                                 const void* scratch, void* out, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = (n + kSelUnit - 1) / kSelUnit;
  static std::atomic<int> occ;
  hipLaunchKernelGGL(ibu_k_select_scatter, dim3(grid_for((u32)nunits, cfg.cus, resident_blocks<kBlock>(cfg, ibu_k_select_scatter, 0, &occ))),
                     dim3(kBlock), 0, st, (const u64*)recs, d_class, (u64)n, (u32)nunits, keep_mask, (const u64*)scratch, (u64*)out);
  return hipGetLastError();
}

}  // namespace ibu
