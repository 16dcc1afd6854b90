// k_matrix.hip — the matrix export (include/ibu_hip.h: ibu_matrix_rows, ibu_matrix_market_body).  Both calls work on the ENTRY TABLE,
// the u64 columns ibu_pair_counts / ibu_count_matrix leave, and both have the shape select has in k_whitelist.hip: a UNIT is 2048
// consecutive entries and belongs to one wave, a count pass leaves one u64 per unit, the single-workgroup scan of kcommon.hpp
// (scan_units_in_place) turns them into offsets with the total in front, and a scatter pass writes.  No workgroup barrier in the
// streaming kernels and no hand-off between workgroups inside a launch.
//   rows: what is counted is the HEADS, the entries whose value differs from the entry before (entry 0 is one); the offsets are row
//         ordinals.
//   text: what is counted is BYTES, the lengths of the decimal lines; the offsets are positions in the text.
// Scratch (matrix_scratch_bytes): u64 [0 .. 2] the maxima of the three printed columns (text only), [3] the total, [4 + u] unit u.
// Behind them, on the same row ordinals: the per-row top-2 (ibu_matrix_row_top) and the class of a row (ibu_assign_rows) — "per-row
// top-2" below.
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
// The same for a value loaded earlier (cur = first[i], 0 past the end): the reduce pass of the per-row top-2 loads rounds ahead.
__device__ __forceinline__ bool mtx_head_of(u64 cur, u64 i, u64 n, u32 lane, u64& carry) {
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

// ---- per-row top-2 ---------------------------------------------------------------------------------------------------
// ibu_matrix_row_top: per row the largest value, the key of the FIRST entry that holds it, the largest value among the other
// entries, the sum and the number of entries — over the entries that TAKE PART (no set: all; a set: the bit of their key is set).
// The row ordinals come from the count + scan of `rows` above; what is new is a segmented reduction whose element is a TUPLE:
//   combine(left, right): the top is the larger value, the LEFT one on equality (so the first entry wins a tie); next = the largest
//   of both `next` and the top that lost; sum and entries add.  The empty tuple (NO_KEY, zeros) is the identity: its zeros lose or
//   tie every unsigned maximum, and a left operand without entries hands the key over whatever the values are.
// reduce   a wave walks its unit in 32 rounds of 64 entries: head ballot (mtx_head), the lane's own tuple, a Hillis-Steele scan over
//          the lanes cut at the heads, and one wave-uniform tuple carried from round to round for the row still open.  A round
//          WITHOUT a head (most rounds where rows are hundreds of entries) ends no row, so it costs no traffic between the lanes:
//          every lane folds its entry into a tuple of its own, and the 64 of them join the open row, in entry order, in front of
//          the next round that has a head or at the unit's end.  A row that
//          opens and closes inside the unit is written at its ordinal by the lane that holds its last entry.  What crosses a seam is
//          left in scratch as two PARTIALS per unit — `head`: the entries in front of the unit's first head (the whole unit if it
//          has none), `tail`: the entries from its last head on — and a flag: has the unit a head?
// finish   one wave per unit that has a head, for the row that begins at the unit's last head: its tail partial, then the head
//          partials of the following units up to and including the first one with a head (that one's is empty when the row ends at
//          the seam).  Lane L takes the units at distance L + 1, L + 65, ... and folds them in order; the 64 lane results are then
//          reduced with the unit number deciding a tied top (the lanes' units interleave).  A row of m entries costs m / 2048
//          partials of 40 B read by one wave, 64 per step: ceil(m / 131072) dependent steps.
// Nothing waits on another workgroup: reduce -> finish is a launch boundary.
// Scratch (row_top_scratch_bytes): the scan array of `rows` (matrix_scratch_bytes), then u64 [c * nunits + u], c = 0 .. 4 the head
// partial of unit u (top, key, next, sum, entries), 5 .. 9 its tail partial, 10 its flag: 88 B per unit.
static constexpr u64 kNoKey = ~0ull;
static constexpr u32 kTopWords = 5, kTopPartialWords = 2 * kTopWords + 1, kTopFinishLanes = kWave;
static constexpr u32 kTopAhead = 4;                // rounds whose loads the reduce pass issues together
static_assert(kMtxRounds % kTopAhead == 0, "whole groups of rounds");

struct Top5 { u64 top, key, next, sum, n; };
__device__ __forceinline__ Top5 top5_empty() { return {0, kNoKey, 0, 0, 0}; }
__device__ __forceinline__ u64 max64(u64 a, u64 b) { return b > a ? b : a; }
__device__ __forceinline__ Top5 top5_combine(const Top5& l, const Top5& r) {
  const bool tr = r.top > l.top || l.n == 0;
  const u64 lost = tr ? l.top : r.top;
  return {tr ? r.top : l.top, tr ? r.key : l.key, max64(max64(l.next, r.next), lost), l.sum + r.sum, l.n + r.n};
}
__device__ __forceinline__ void top5_store(u64* __restrict__ part, u32 nunits, u32 u, u32 c0, const Top5& t) {
  part[(size_t)(c0 + 0) * nunits + u] = t.top;
  part[(size_t)(c0 + 1) * nunits + u] = t.key;
  part[(size_t)(c0 + 2) * nunits + u] = t.next;
  part[(size_t)(c0 + 3) * nunits + u] = t.sum;
  part[(size_t)(c0 + 4) * nunits + u] = t.n;
}
__device__ __forceinline__ Top5 top5_load(const u64* __restrict__ part, u32 nunits, u32 u, u32 c0) {
  return {part[(size_t)(c0 + 0) * nunits + u], part[(size_t)(c0 + 1) * nunits + u], part[(size_t)(c0 + 2) * nunits + u],
          part[(size_t)(c0 + 3) * nunits + u], part[(size_t)(c0 + 4) * nunits + u]};
}
// Tuples whose entries are NOT adjacent in lane order (a lane that folds every 64th entry, or every 64th unit) carry the POSITION of
// their top beside them: `at`, ~0 while there are no entries.  A lane folds in ascending position, so the left operand wins a tie;
// across the lanes the smaller position does.
__device__ __forceinline__ void top5_fold(Top5& acc, u32& at, const Top5& t, u32 pos) {
  const bool tr = t.n != 0 && (t.top > acc.top || acc.n == 0);
  at = tr ? pos : at;
  acc = top5_combine(acc, t);
}
// The 64 lane tuples -> their combination in position order, in every lane.
__device__ __forceinline__ void top5_reduce_by_position(Top5& acc, u32& at) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const Top5 o{shfl_xor64(acc.top, m), shfl_xor64(acc.key, m), shfl_xor64(acc.next, m), shfl_xor64(acc.sum, m), shfl_xor64(acc.n, m)};
    const u32 oat = __shfl_xor(at, m);
    const bool to = o.top > acc.top || (o.top == acc.top && oat < at);   // an operand without entries has top 0 and at = ~0
    const u64 lost = to ? acc.top : o.top;
    acc = {to ? o.top : acc.top, to ? o.key : acc.key, max64(max64(acc.next, o.next), lost), acc.sum + o.sum, acc.n + o.n};
    at = to ? oat : at;
  }
}
struct TopOut { u64* key; u64* top; u64* next; u64* sum; u64* n; };   // each nullable
__device__ __forceinline__ void top5_write(const TopOut& o, u64 r, const Top5& t) {
  if (o.key) o.key[r] = t.key;
  if (o.top) o.top[r] = t.top;
  if (o.next) o.next[r] = t.next;
  if (o.sum) o.sum[r] = t.sum;
  if (o.n) o.n[r] = t.n;
}

// (Three waves per SIMD: the scanned tuple, the open row, the tuple a lane holds and the columns of four rounds take 149 registers;
// with one round's columns it was 134, and bounded to the 128 of four waves that build kept 28 B per lane in scratch memory.)
extern "C" __global__ void __launch_bounds__(kBlock, 3)
ibu_k_rowtop_reduce(const u64* __restrict__ first, const u64* __restrict__ second, const u64* __restrict__ values, u64 n, u32 nunits,
                     const u64* __restrict__ set /*nullable*/, u64 set_bits, const u64* __restrict__ units, TopOut out,
                     u64* __restrict__ part) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  const u64 upto = ~0ull >> (63 - lane);           // this lane and the lanes below it
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    const u64 base = (u64)u * kMtxUnit;
    u64 hcarry = base ? first[base - 1] : 0;
    u64 pos = units[1 + u];                        // heads in front of this unit
    Top5 open = top5_empty();                      // wave-uniform: the row still open behind the rounds so far
    bool seen = false;                             // wave-uniform: the unit has had a head
    Top5 held = top5_empty();                      // per lane: its entries of the rounds without a head since the last round with one
    u32 held_at = ~0u;
    bool holding = false;                          // wave-uniform
    // kTopAhead rounds at a time: their twelve loads go out together, then their gathered bitmap words, then the rounds are worked
    // through in order (one round's three loads in flight per wave, at three waves, left the memory idle)
#pragma unroll 1
    for (u32 r0 = 0; r0 < kMtxRounds; r0 += kTopAhead) {
      u64 cur_a[kTopAhead], key_a[kTopAhead], val_a[kTopAhead];
      bool in_a[kTopAhead];
#pragma unroll
      for (u32 j = 0; j < kTopAhead; ++j) {
        const u64 i = base + (r0 + j) * kWave + lane;
        cur_a[j] = i < n ? __builtin_nontemporal_load(first + i) : 0;
        key_a[j] = i < n ? __builtin_nontemporal_load(second + i) : 0;
        val_a[j] = i < n ? __builtin_nontemporal_load(values + i) : 0;
      }
#pragma unroll
      for (u32 j = 0; j < kTopAhead; ++j) {
        const u64 k = key_a[j];
        in_a[j] = base + (r0 + j) * kWave + lane < n;
        if (set) in_a[j] = in_a[j] && k < set_bits && ((set[k >> 6] >> (k & 63)) & 1) != 0;   // one gathered word; `set` is wave-uniform
      }
#pragma unroll
      for (u32 j = 0; j < kTopAhead; ++j) {
        const u32 r = r0 + j;
        const u64 i = base + r * kWave + lane;
        const bool head = mtx_head_of(cur_a[j], i, n, lane, hcarry);
        const u64 b = __ballot(head);
        const u64 key = key_a[j], val = val_a[j];
        const bool in = in_a[j];
        if (b == 0) {                              // wave-uniform: no row ends here, so nothing across the lanes is due yet
          top5_fold(held, held_at, in ? Top5{val, key, 0, val, 1} : top5_empty(), r * kWave + lane);
          holding = true;
          continue;
        }
        if (holding) {                               // the open row takes what the lanes hold, in entry order
          top5_reduce_by_position(held, held_at);
          open = top5_combine(open, held);
          held = top5_empty();
          held_at = ~0u;
          holding = false;
        }
        const u64 p = __ballot(in);
        // the lane's segment inside the round begins at the last head at or below it, or at lane 0 (the open row goes on)
        const u64 hb = b & upto;
        const u32 start = hb ? 63u - (u32)__builtin_clzll(hb) : 0u;
        // the scanned tuple: top, next, sum, and the LANE that holds the top (64: none) — the key is fetched once, behind the scan
        u64 top = in ? val : 0, next = 0, sum = top;
        u32 src = in ? lane : 64u;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
          const u64 ftop = shfl_up64(top, d), fnext = shfl_up64(next, d), fsum = shfl_up64(sum, d);
          const u32 fsrc = __shfl_up(src, d);
          if (lane >= (u32)d && lane - (u32)d >= start) {          // combine(front, own)
            const bool own = top > ftop || fsrc == 64u;
            const u64 lost = own ? ftop : top;
            next = max64(max64(fnext, next), lost);
            top = own ? top : ftop;
            src = own ? src : fsrc;
            sum += fsum;
          }
        }
        const u64 skey = shfl64(key, (int)(src & 63u));
        Top5 t{top, src == 64u ? kNoKey : skey, next, sum, (u64)__builtin_popcountll(p & upto & (~0ull << start))};
        if (!hb) t = top5_combine(open, t);          // no head at or below this lane: the open row reaches into the round
        // a head at lane 0 closes the open row as it stands; a head at lane L + 1 closes the row of lane L
        const bool closes = lane < kWave - 1 && ((b >> (lane + 1)) & 1) != 0;
        if (closes) {
          if (seen || hb) top5_write(out, pos + (u32)__builtin_popcountll(hb) - 1, t);
          else top5_store(part, nunits, u, 0, t);    // the row began in front of the unit: the head partial
        }
        if ((b & 1) && lane == 0) {
          if (seen) top5_write(out, pos - 1, open);
          else top5_store(part, nunits, u, 0, open);
        }
        // the new open row: what lane 63 holds (entries past n take no part and are no heads)
        open = {shfl64(t.top, kWave - 1), shfl64(t.key, kWave - 1), shfl64(t.next, kWave - 1), shfl64(t.sum, kWave - 1),
                shfl64(t.n, kWave - 1)};
        seen = seen || b != 0;
        pos += (u32)__builtin_popcountll(b);
      }
    }
    if (holding) {
      top5_reduce_by_position(held, held_at);
      open = top5_combine(open, held);
    }
    if (lane == 0) {
      if (seen) top5_store(part, nunits, u, kTopWords, open);
      else top5_store(part, nunits, u, 0, open);
      part[(size_t)(2 * kTopWords) * nunits + u] = seen ? 1 : 0;
    }
  }
}

extern "C" __global__ void __launch_bounds__(kBlock, 8)
ibu_k_rowtop_finish(u32 nunits, const u64* __restrict__ units, const u64* __restrict__ part, TopOut out) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 nwaves = gridDim.x * kWavesPerBlock;
  const u64* __restrict__ flag = part + (size_t)(2 * kTopWords) * nunits;
  for (u32 u = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nunits; u += nwaves) {
    if (!flag[u]) continue;                        // wave-uniform: no row begins in this unit
    Top5 acc = lane == 0 ? top5_load(part, nunits, u, kTopWords) : top5_empty();
    u32 at = acc.n ? u : ~0u;                      // the unit the top comes from; no entries: behind every unit
    for (u32 v0 = u + 1; v0 < nunits; v0 += kTopFinishLanes) {   // wave-uniform
      const u32 v = v0 + lane;
      const bool valid = v < nunits;
      const u64 fb = __ballot(valid && flag[v] != 0);
      // the units up to and including the first one with a head
      if (valid && (fb == 0 || lane <= (u32)__builtin_ctzll(fb))) top5_fold(acc, at, top5_load(part, nunits, v, 0), v);
      if (fb) break;
    }
    top5_reduce_by_position(acc, at);
    // the ordinal of the unit's last head: the heads in front of the next unit, less one
    if (lane == 0) top5_write(out, (u + 1 < nunits ? units[2 + u] : units[0]) - 1, acc);
  }
}

// ---- the class of a row ----------------------------------------------------------------------------------------------
// ibu_assign_rows: elementwise over the columns ibu_matrix_row_top leaves.  The share test top * den >= num * sum is taken in 128 bits.
// acc (nullable, uniform over the grid; block_accumulate): rows per class [0 .. 2].
struct AssignRule { u64 min_value, num, den; };
__device__ __forceinline__ bool mul_ge(u64 a, u64 b, u64 c, u64 d) {   // a * b >= c * d, exactly
  const u64 h1 = __umul64hi(a, b), h2 = __umul64hi(c, d);
  return h1 != h2 ? h1 > h2 : a * b >= c * d;
}
extern "C" __global__ void __launch_bounds__(kBlock)
ibu_k_rowtop_assign(const u64* __restrict__ top, const u64* __restrict__ next, const u64* __restrict__ sum, u64 rows, AssignRule rule,
                    uint8_t* __restrict__ cls_out /*nullable*/, u64* __restrict__ acc /*nullable*/) {
  __shared__ u64 accl[kWavesPerBlock * 3];
  const u64 floor = rule.min_value ? rule.min_value : 1;
  u64 t[3] = {0, 0, 0};
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < rows; k += stride) {
    const u64 tv = top[k], nv = next[k], sv = sum[k];
    const u32 c = tv < floor ? 1u : (tv > nv && (rule.num == 0 || mul_ge(tv, rule.den, rule.num, sv))) ? 0u : 2u;
    if (cls_out) cls_out[k] = (uint8_t)c;
#pragma unroll
    for (u32 q = 0; q < 3; ++q) t[q] += c == q ? 1 : 0;
  }
  if (!acc) return;                                // uniform over the grid
  block_accumulate(t, acc, accl);
}

// ---- launchers -------------------------------------------------------------------------------------------------------
static inline u64 mtx_units(size_t n) { return (n + kMtxUnit - 1) / kMtxUnit; }
size_t matrix_scratch_bytes(size_t n) { return 8 * (kMtxHead + 1 + mtx_units(n)); }
size_t row_top_scratch_bytes(size_t n) { return matrix_scratch_bytes(n) + 8 * kTopPartialWords * mtx_units(n); }
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
// Behind launch_matrix_rows_count on the same scratch (row_top_scratch_bytes(n) of it): the reduce pass and the finishing pass.
hipError_t launch_matrix_row_top(const LaunchCfg& cfg, const uint64_t* first, const uint64_t* second, const uint64_t* values, size_t n,
                                 const uint64_t* set, uint64_t set_bits, void* scratch, size_t scratch_bytes, uint64_t* top_key,
                                 uint64_t* top_value, uint64_t* next_value, uint64_t* row_sum, uint64_t* row_entries, hipStream_t st) {
  (void)hipGetLastError();
  if (n == 0) return hipSuccess;
  const u64 nunits = mtx_units(n);
  if (nunits > 0xFFFFFFFFull || scratch_bytes < row_top_scratch_bytes(n) || (!set && set_bits)) return hipErrorInvalidValue;
  u64* part = (u64*)((uint8_t*)scratch + matrix_scratch_bytes(n));
  const TopOut out{(u64*)top_key, (u64*)top_value, (u64*)next_value, (u64*)row_sum, (u64*)row_entries};
  hipLaunchKernelGGL(ibu_k_rowtop_reduce, dim3(tiled_grid<ibu_k_rowtop_reduce>(cfg, (u32)nunits)), dim3(kBlock), 0, st, (const u64*)first,
                     (const u64*)second, (const u64*)values, (u64)n, (u32)nunits, (const u64*)set, (u64)set_bits,
                     (const u64*)mtx_scan_array(scratch), out, part);
  hipLaunchKernelGGL(ibu_k_rowtop_finish, dim3(tiled_grid<ibu_k_rowtop_finish>(cfg, (u32)nunits)), dim3(kBlock), 0, st,
                     (u32)nunits, (const u64*)mtx_scan_array(scratch), (const u64*)part, out);
  return hipGetLastError();
}
hipError_t launch_matrix_assign(const LaunchCfg& cfg, const uint64_t* top_value, const uint64_t* next_value, const uint64_t* row_sum,
                                size_t rows, uint64_t min_value, uint64_t num, uint64_t den, uint8_t* d_class, uint64_t* acc, hipStream_t st) {
  (void)hipGetLastError();
  if (den == 0 || num > den || (!d_class && !acc)) return hipErrorInvalidValue;
  const hipError_t e = zero_totals(acc, 3, st);
  if (e != hipSuccess || rows == 0) return e;
  hipLaunchKernelGGL(ibu_k_rowtop_assign, dim3(capped_grid(cfg, rows, kBlock)), dim3(kBlock), 0, st, (const u64*)top_value,
                     (const u64*)next_value, (const u64*)row_sum, (u64)rows, AssignRule{min_value, num, den}, d_class, (u64*)acc);
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
