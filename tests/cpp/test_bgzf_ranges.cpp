// The ranges of the pull stream over a BGZF file (ibu_stream_open_path; ibu_amd/csrc/bgzf_plan.hpp: plan_range_records, plan_records) on
// one file, printed as JSON lines for tests/test_bgzf_ranges.py:
//   test_bgzf_ranges <file> <slot_records,...> <target_bytes,...> [noshards]
// first the index, then the plan of every shard for n_shards 1 .. 9 (plan_shard, as tests/cpp/test_bgzf_plan.cpp prints it), then for
// every slot size and range target the range size and the plan of every range, each with the CRC-32 of the range's bytes as this driver
// puts them together from the plan alone (header bytes, edge blocks and device blocks, every block inflated by inflate_block_on_host).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "bgzf_plan.hpp"

using namespace ibu;

namespace {

std::vector<uint8_t> buf;
BgzfIndex idx;

std::vector<size_t> numbers(const char* s) {
  std::vector<size_t> v;
  for (const char* p = s; *p;) {
    char* end = nullptr;
    v.push_back((size_t)strtoull(p, &end, 10));
    p = *end ? end + 1 : end;
  }
  return v;
}

// The plan's fields and the CRC-32 of the bytes it puts together
void print_plan(const ShardPlan& p, const char* lead) {
  pgz::RawInflater raw;
  std::vector<uint8_t> bytes(p.hi - p.lo, 0), out(65536);
  auto put = [&](const uint8_t* b, uint64_t at, uint64_t len) {
    for (uint64_t a = at < p.lo ? p.lo : at; a < at + len && a < p.hi; ++a) bytes[a - p.lo] = b[a - at];
  };
  put(idx.head.data(), 0, idx.head.size());
  auto put_block = [&](size_t j) {
    const ibu_inflate_block_t& b = idx.blocks[j];
    if (inflate_block_on_host(raw, buf.data(), b, out.data())) {
      ibu_error_detail_t d;
      ibu_last_error(&d);
      fprintf(stderr, "block %zu: %s\n", j, d.message);
      exit(1);
    }
    put(out.data(), (uint64_t)b.out_offset, b.out_len);
  };
  printf("%s\"rec_first\": %zu, \"num\": %zu, \"lo\": %llu, \"hi\": %llu, \"dev_first\": %zu, \"dev_end\": %zu, \"edges\": [", lead, p.rec_first, p.num,
         (unsigned long long)p.lo, (unsigned long long)p.hi, p.dev_first, p.dev_end);
  for (size_t e = 0; e < p.n_edges; ++e) {
    printf("%s%zu", e ? ", " : "", p.edge[e]);
    put_block(p.edge[e]);
  }
  for (size_t j = p.dev_first; j < p.dev_end; ++j) put_block(j);
  printf("], \"cbeg\": %zu, \"cend\": %zu, \"crc\": %lu}", p.cbeg, p.cend, crc32(0, bytes.data(), (uInt)bytes.size()));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) { fprintf(stderr, "usage: %s <file> <slot_records,...> <target_bytes,...> [noshards]\n", argv[0]); return 2; }
  if (FILE* f = fopen(argv[1], "rb")) {
    uint8_t chunk[1 << 16];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + k);
    fclose(f);
  } else {
    perror(argv[1]);
    return 2;
  }
  const int32_t rc = bgzf_index(buf.data(), buf.size(), &idx);
  printf("{\"rc\": %d, \"total\": %llu, \"lead\": %zu, \"head\": %zu, \"file_bytes\": %zu, \"blocks\": [", rc, (unsigned long long)idx.total, idx.lead,
         idx.head.size(), idx.file_bytes);
  for (size_t i = 0; i < idx.blocks.size(); ++i) {
    const ibu_inflate_block_t& b = idx.blocks[i];
    printf("%s[%llu, %u, %lld, %u, %u]", i ? ", " : "", (unsigned long long)b.comp_offset, b.comp_len, (long long)b.out_offset, b.out_len, b.crc32);
  }
  printf("]}\n");
  if (rc) return 0;
  for (size_t k = 1; k <= 9 && argc == 4; ++k) {
    for (size_t i = 0; i < k; ++i) {
      ShardPlan p;
      if (plan_shard(idx, i, k, &p)) return 1;
      char lead[64];
      snprintf(lead, sizeof lead, "{\"n_shards\": %zu, \"shard\": %zu, ", k, i);
      print_plan(p, lead);
      printf("\n");
    }
  }
  const size_t total = (size_t)((idx.total - IBU_HEADER_SIZE) / IBU_RECORD_SIZE);
  for (size_t slot : numbers(argv[2])) {
    for (size_t target : numbers(argv[3])) {
      const size_t r = plan_range_records(idx, target, slot);
      printf("{\"slot\": %zu, \"target\": %zu, \"range_records\": %zu, \"ranges\": [", slot, target, r);
      for (size_t first = 0, k = 0; first < total; first += r, ++k) {
        ShardPlan p;
        if (plan_records(idx, first, total - first < r ? total - first : r, &p)) return 1;
        print_plan(p, k ? ", {" : "{");
      }
      printf("]}\n");
    }
  }
  ShardPlan p;                                           // records past the end are refused
  printf("{\"past_end\": %d}\n", plan_records(idx, total, 1, &p));
  return 0;
}
