// The shared argument checks of the C ABI's entry points (ibu_amd/csrc/api_checks.hpp) on the host: one JSON line per case, asserted by
// tests/test_api_checks.py.  Plain g++, no GPU.  A check that sets an error is read back through ibu_last_error, as a caller would.
#include <stdint.h>
#include <stdio.h>

#include "api_checks.hpp"

static void status(const char* name, int32_t rc) {
  ibu_error_detail_t d;
  ibu_last_error(&d);
  if (rc == IBU_OK)
    printf("{\"case\": \"%s\", \"rc\": 0}\n", name);
  else
    printf("{\"case\": \"%s\", \"rc\": %d, \"status\": \"%s\", \"code\": %d, \"a\": %llu, \"b\": %llu, \"message\": \"%s\"}\n", name, rc,
           ibu_status_name(rc), d.code, (unsigned long long)d.a, (unsigned long long)d.b, d.message);
}
static void overlap(const char* name, uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) {
  const bool ab = ibu::ranges_overlap(reinterpret_cast<const void*>(a), a_bytes, reinterpret_cast<const void*>(b), b_bytes);
  const bool ba = ibu::ranges_overlap(reinterpret_cast<const void*>(b), b_bytes, reinterpret_cast<const void*>(a), a_bytes);
  printf("{\"case\": \"%s\", \"overlap\": %s, \"swapped\": %s}\n", name, ab ? "true" : "false", ba ? "true" : "false");
}

int main() {
  const uintptr_t top = UINTPTR_MAX;
  overlap("disjoint", 0x1000, 24, 0x2000, 24);
  overlap("adjacent", 0x1000, 24, 0x1018, 24);
  overlap("one_shared_byte", 0x1000, 25, 0x1018, 24);
  overlap("inside", 0x1000, 240, 0x1030, 24);
  overlap("identical", 0x1000, 24, 0x1000, 24);
  overlap("first_empty", 0x1008, 0, 0x1000, 24);
  overlap("both_empty", 0x1000, 0, 0x1000, 0);
  overlap("ends_at_top_disjoint", top - 23, 24, 0x1000, 24);       // top - 23 + 24 wraps to 0 when the end is formed
  overlap("ends_at_top_adjacent", top - 23, 24, top - 47, 24);
  overlap("ends_at_top_shared", top - 23, 24, top - 46, 24);
  overlap("huge_length_from_low", 0x1000, (size_t)top - 0x1000 + 1, top - 7, 8);   // [0x1000, 2^64): holds the last 8 bytes

  alignas(8) static unsigned char words[16];
  status("ptr_null", ibu::check_u64_ptr(nullptr, "d_records"));
  status("ptr_mod8_0", ibu::check_u64_ptr(words, "d_records"));
  status("ptr_mod8_1", ibu::check_u64_ptr(words + 1, "d_sorted_records"));
  status("ptr_mod8_4", ibu::check_u64_ptr(words + 4, "d_codes"));
  status("ptrs_both_good", ibu::check_u64_ptrs({words, words + 8}, "d_records / d_tmp"));
  status("ptrs_second_null", ibu::check_u64_ptrs({words, nullptr}, "d_records / d_tmp"));
  status("ptrs_second_mod8_4", ibu::check_u64_ptrs({words, words + 4}, "d_a / d_b"));
  printf("{\"case\": \"aligned8\", \"values\": [%d, %d, %d, %d]}\n", ibu::aligned8(nullptr), ibu::aligned8(words), ibu::aligned8(words + 1),
         ibu::aligned8(words + 4));

  status("limit_just_below", ibu::check_below_2_40((1ull << 40) - 1, "sort_records", "records"));
  status("limit_at", ibu::check_below_2_40(1ull << 40, "sort_records", "records"));
  status("limit_size_max", ibu::check_below_2_40(SIZE_MAX, "subsample_class", "rows"));
  status("limit_values", ibu::check_below_2_40(1ull << 40, "rank_select", "values"));
  status("limit_codes", ibu::check_below_2_40(1ull << 41, "abundance_counts", "codes"));

  status("capacity_pairs", ibu::err_capacity(12, 11, "entries", "n_pairs"));
  status("capacity_select", ibu::err_capacity(64, 63, "records kept", "n_out"));
  status("capacity_metrics", ibu::err_capacity(1ull << 33, 7, "barcodes", "n_barcodes"));
  return 0;
}
