// The host half of the BGZF device load (ibu_amd/csrc/bgzf_plan.hpp) on one file, printed as JSON lines for tests/test_bgzf_plan.py:
//   test_bgzf_plan <file> <pieces_min_bytes>
// first the index, then the plan of every shard for n_shards 1 .. 9, each with the CRC-32 of the shard's bytes as this driver puts them
// together from the plan alone (header bytes, edge blocks and device blocks, every block inflated by inflate_block_on_host).
#include <stdio.h>
#include <stdlib.h>
#include <zlib.h>

#include <vector>

#include "bgzf_plan.hpp"

using namespace ibu;

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <file> <pieces_min_bytes>\n", argv[0]); return 2; }
  std::vector<uint8_t> buf;
  if (FILE* f = fopen(argv[1], "rb")) {
    uint8_t chunk[1 << 16];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + k);
    fclose(f);
  } else {
    perror(argv[1]);
    return 2;
  }
  BgzfIndex idx;
  const int32_t rc = bgzf_index(buf.data(), buf.size(), &idx, strtoull(argv[2], nullptr, 10));
  printf("{\"rc\": %d, \"total\": %llu, \"lead\": %zu, \"head\": %zu, \"in_pieces\": %d, \"blocks\": [", rc, (unsigned long long)idx.total, idx.lead,
         idx.head.size(), (int)idx.in_pieces);
  for (size_t i = 0; i < idx.blocks.size(); ++i) {
    const ibu_inflate_block_t& b = idx.blocks[i];
    printf("%s[%llu, %u, %lld, %u, %u]", i ? ", " : "", (unsigned long long)b.comp_offset, b.comp_len, (long long)b.out_offset, b.out_len, b.crc32);
  }
  printf("]}\n");
  if (rc) return 0;
  pgz::RawInflater raw;
  std::vector<uint8_t> shard, out(65536);
  for (size_t k = 1; k <= 9; ++k) {
    for (size_t i = 0; i < k; ++i) {
      ShardPlan p;
      if (plan_shard(idx, i, k, &p)) return 1;
      shard.assign(p.hi - p.lo, 0);
      auto put = [&](const uint8_t* bytes, uint64_t at, uint64_t len) {
        for (uint64_t a = at < p.lo ? p.lo : at; a < at + len && a < p.hi; ++a) shard[a - p.lo] = bytes[a - at];
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
      printf("{\"n_shards\": %zu, \"shard\": %zu, \"rec_first\": %zu, \"num\": %zu, \"lo\": %llu, \"hi\": %llu, \"dev_first\": %zu, \"dev_end\": %zu, "
             "\"edges\": [", k, i, p.rec_first, p.num, (unsigned long long)p.lo, (unsigned long long)p.hi, p.dev_first, p.dev_end);
      for (size_t e = 0; e < p.n_edges; ++e) {
        printf("%s%zu", e ? ", " : "", p.edge[e]);
        put_block(p.edge[e]);
      }
      for (size_t j = p.dev_first; j < p.dev_end; ++j) put_block(j);
      printf("], \"cbeg\": %zu, \"cend\": %zu, \"crc\": %lu}\n", p.cbeg, p.cend, crc32(0, shard.data(), (uInt)shard.size()));
    }
  }
  return 0;
}
