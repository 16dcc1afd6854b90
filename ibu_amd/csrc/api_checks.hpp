// api_checks.hpp — the argument checks the entry points of the C ABI share (device.cpp, api_*.cpp).  Host arithmetic on top of
// common.hpp only: no HIP, so that tests/cpp/test_api_checks.cpp drives every one of them with plain g++.  The helpers that need the
// context (check_ctx, read_back) are in ctx.hpp.  Each message is the ABI's, byte for byte: a wording that fits none of these stays
// written out at its call site.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "common.hpp"

namespace ibu {

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// A device array of u64 words (records, codes, columns).  `what`: the argument's name, or the names of several as their message
// lists them ("d_records / d_tmp").
inline int32_t check_u64_ptrs(std::initializer_list<const void*> ps, const char* what) {
  for (const void* p : ps)
    if (!p || !aligned8(p))
      return set_error(IBU_ERR_INVALID_ARG, 0, 0, 0, "Invalid argument: %s must be non-NULL and 8-byte aligned", what);
  return IBU_OK;
}
inline int32_t check_u64_ptr(const void* p, const char* what) { return check_u64_ptrs({p}, what); }

// The kernels index rows with 40 bits: an argument limit, not a HIP error.  `what`: records, rows, values, codes.
inline int32_t check_below_2_40(uint64_t n, const char* fn, const char* what) {
  if (n < (1ull << 40)) return IBU_OK;
  return set_error(IBU_ERR_INVALID_ARG, 0, 0, 0, "Invalid argument: %s handles fewer than 2^40 %s per call", fn, what);
}

// An argument that stands for one byte (a label, a class): a = the value.  `what`: fill, match, missing_class, missing.
inline int32_t check_byte(uint32_t v, const char* what) {
  if (v <= 255u) return IBU_OK;
  return set_error(IBU_ERR_INVALID_ARG, v, 0, 0, "Invalid argument: %s must be at most 255 (it stands for one byte)", what);
}

// Do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  An empty range shares none.  Compares distances, never an end: a range
// that ends at the top of the address space does not wrap.
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (a_bytes == 0 || b_bytes == 0) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa <= pb ? pb - pa < a_bytes : pa - pb < b_bytes;
}

// The second half of the size-query protocol: the outputs hold `cap` entries and the call needs `need` (a = need, b = cap).
// `what` / `see`: "entries" / "n_pairs", "records kept" / "n_out", "barcodes" / "n_barcodes".
inline int32_t err_capacity(uint64_t need, uint64_t cap, const char* what, const char* see) {
  return set_error(IBU_ERR_INVALID_ARG, need, cap, 0, "Invalid argument: output capacity %llu is smaller than the %llu %s (see *%s)",
                   (unsigned long long)cap, (unsigned long long)need, what, see);
}

}  // namespace ibu
