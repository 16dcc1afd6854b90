// partition_plan.hpp — how ibu_partition_records cuts n records and n_parts parts into units (k_partition.hip, api_whitelist.cpp).
// Host arithmetic only: no HIP, so that a CPU test compiles it with plain g++.
//
// A UNIT is `unit` consecutive records and belongs to one wave.  The table holds one u64 per (part, unit), part-major, behind one
// word for the total: table[0] = records kept, table[1 + p * nunits + u] = the records of part p in unit u and, after ONE exclusive
// scan of the flattened table, the first output position of that part's records of that unit.  Behind the table n_parts + 1 words
// take the part starts and the total, gathered for the read-back.
//
//   unit    = max(2048, the power of two at or above 64 * n_parts)          (2048 is select's unit; 255 parts: 16384)
//   nunits  = ceil(n / unit)
//   entries = n_parts * nunits                                              (the scanned length: must fit the scan's u32)
//   scratch = 8 * (1 + entries + n_parts + 1) bytes  <=  n / 8 + kPartitionScratchConst
// because 8 * n_parts * nunits < 8 * n_parts * (n / unit + 1) and unit >= 64 * n_parts: the table never takes more than an eighth
// of a byte per record plus 8 * n_parts, whatever n_parts is.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ibu {

static constexpr uint32_t kPartitionMinUnit = 2048;     // select's kSelUnit
static constexpr uint32_t kPartitionMaxParts = 255;
static constexpr uint32_t kPartitionNone = 255;         // IBU_PART_NONE
static constexpr size_t kPartitionScratchConst = 8 * (2 + 2 * 255);   // 8 * n_parts of rounding, the total, n_parts + 1 gathered words
// The scan walks the table in steps of 16384 entries with a u32 cursor: the step behind the last one must not wrap.
static constexpr uint64_t kPartitionMaxEntries = 0xFFFFFFFFull - 16384;

struct PartitionPlan {
  uint32_t unit = 0;        // records per unit: a power of two, at least kPartitionMinUnit
  uint64_t nunits = 0;
  uint64_t entries = 0;     // n_parts * nunits: the table behind its first word
  size_t scratch_bytes = 0;
  bool ok = false;          // false: n_parts outside 1 .. 255, or more entries than the scan takes
};

inline uint32_t partition_unit(uint32_t n_parts) {
  uint32_t unit = kPartitionMinUnit;
  while (unit < 64u * n_parts) unit <<= 1;
  return unit;
}

inline PartitionPlan partition_plan(uint64_t n, uint32_t n_parts) {
  PartitionPlan p;
  if (n_parts < 1 || n_parts > kPartitionMaxParts) return p;
  p.unit = partition_unit(n_parts);
  p.nunits = n / p.unit + (n % p.unit != 0);
  p.entries = (uint64_t)n_parts * p.nunits;
  p.scratch_bytes = (size_t)(8 * (1 + p.entries + n_parts + 1));
  p.ok = p.entries <= kPartitionMaxEntries;
  return p;
}

}  // namespace ibu
