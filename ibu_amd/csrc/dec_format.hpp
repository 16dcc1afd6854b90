// dec_format.hpp — the shortest decimal form of a 64-bit unsigned value, as arithmetic only: how many digits, and which.  Compiles
// for host and device and uses neither HIP types nor LDS, so that tests/test_mtx_host.py drives it with plain g++ against snprintf;
// k_matrix.hip (ibu_matrix_market_body) is the user.  No division by anything but a constant, and no per-value digit array: a
// caller says where digit k goes (dec_emit's `put`), so a kernel writes straight into its staging area and keeps nothing indexed at
// run time in registers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IBU_DEC_HD __host__ __device__ __forceinline__
#else
#define IBU_DEC_HD inline
#endif

namespace ibu {

// The number of decimal digits of a 32-bit x, 1 .. 10 (0 has one): nine comparisons against the powers of ten.
IBU_DEC_HD uint32_t dec_digits32(uint32_t x) {
  uint32_t n = 1;
  n += x >= 10u;
  n += x >= 100u;
  n += x >= 1000u;
  n += x >= 10000u;
  n += x >= 100000u;
  n += x >= 1000000u;
  n += x >= 10000000u;
  n += x >= 100000000u;
  n += x >= 1000000000u;
  return n;
}
// ... and of a 64-bit v, 1 .. 20, branch-free: nineteen 64-bit comparisons.  A caller that knows a whole batch of values to be below
// 2^32 (indices, ordinals and counts nearly always are) takes dec_digits32 for the batch instead.
IBU_DEC_HD uint32_t dec_digits(uint64_t v) {
  uint32_t n = 1;
  n += v >= 10ull;
  n += v >= 100ull;
  n += v >= 1000ull;
  n += v >= 10000ull;
  n += v >= 100000ull;
  n += v >= 1000000ull;
  n += v >= 10000000ull;
  n += v >= 100000000ull;
  n += v >= 1000000000ull;
  n += v >= 10000000000ull;
  n += v >= 100000000000ull;
  n += v >= 1000000000000ull;
  n += v >= 10000000000000ull;
  n += v >= 100000000000000ull;
  n += v >= 1000000000000000ull;
  n += v >= 10000000000000000ull;
  n += v >= 100000000000000000ull;
  n += v >= 1000000000000000000ull;
  n += v >= 10000000000000000000ull;
  return n;
}

// v = (hi * 10^9 + mid) * 10^9 + lo with lo, mid < 10^9 and hi <= 18: two divisions by a constant.
IBU_DEC_HD void dec_chunks(uint64_t v, uint32_t& lo, uint32_t& mid, uint32_t& hi) {
  const uint64_t q = v / 1000000000ull;
  lo = (uint32_t)(v - q * 1000000000ull);
  hi = (uint32_t)(q / 1000000000ull);
  mid = (uint32_t)(q - (uint64_t)hi * 1000000000ull);
}

// x / 10 for any 32-bit x: one 32 x 32 -> 64 multiply and a shift (0xCCCCCCCD = ceil(2^35 / 10)).
IBU_DEC_HD uint32_t dec_div10(uint32_t x) { return (uint32_t)(((uint64_t)x * 0xCCCCCCCDu) >> 35); }

// The low `count` digits of a chunk, least significant first: put(first + k, '0' + digit k) for every k < count with first + k < nd.
template <int COUNT, class Put>
IBU_DEC_HD void dec_emit_chunk(uint32_t x, uint32_t first, uint32_t nd, Put& put) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < COUNT; ++k) {
    const uint32_t q = dec_div10(x);
    if (first + (uint32_t)k < nd) put(first + (uint32_t)k, (char)('0' + (x - 10u * q)));
    x = q;
  }
}

// The nd = dec_digits(v) digits of v: put(k, c) is called once for every k < nd, c being the digit of 10^k — the LAST character of
// the text is k = 0.  The chunks above the first are not touched while nd <= 9, the third not while nd <= 18.
template <class Put>
IBU_DEC_HD void dec_emit(uint64_t v, uint32_t nd, Put put) {
  if (nd <= 9) {
    dec_emit_chunk<9>((uint32_t)v, 0, nd, put);
    return;
  }
  uint32_t lo, mid, hi;
  dec_chunks(v, lo, mid, hi);
  dec_emit_chunk<9>(lo, 0, nd, put);
  dec_emit_chunk<9>(mid, 9, nd, put);
  if (nd > 18) dec_emit_chunk<2>(hi, 18, nd, put);
}

}  // namespace ibu
