// bgzf_plan.hpp — the host half of the BGZF device load (stream.cpp): the index of a file's blocks and the plan of one shard of it.
#pragma once
#include "../../include/ibu_hip.h"
#include "pgzip.hpp"

namespace ibu {

// The decoder's short form takes this many blocks in one round (three waves of 64 blocks per CU); a load of more launches ahead.
inline size_t inflate_one_round(uint32_t cus) { return (size_t)cus * 3 * 64; }

struct BgzfIndex {
  std::vector<ibu_inflate_block_t> blocks;
  uint64_t total = 0;                        // the inflated stream's bytes
  size_t file_bytes = 0, lead = 0;           // blocks [0, lead) hold the 32 header bytes, inflated on the host to `head`
  std::vector<uint8_t> head;
  ibu_header_t header{};
  bool in_pieces = false;                    // the walk in eight pieces was used (files from pieces_min_bytes on)
};
// The blocks of map[0, size) (a cut-off or foreign member: IBU_ERR_NIFFLER), the header validated, whole records checked.
int32_t bgzf_index(const uint8_t* map, size_t size, BgzfIndex* idx, size_t pieces_min_bytes = (size_t)32 << 20);
// Block b inflated to out[0, b.out_len) and checked against its length and CRC-32 (else IBU_ERR_NIFFLER, as from the Reader).
int32_t inflate_block_on_host(pgz::RawInflater& raw, const uint8_t* map, const ibu_inflate_block_t& b, uint8_t* out);

// Shard `shard` of `n_shards` of the records (ibu_shard_range): the blocks wholly inside its bytes [lo, hi) go to the device, the (at
// most two) that straddle its ends are inflated on the host, as the header's blocks are.  File bytes [cbeg, cend) cross the link.
struct ShardPlan {
  size_t rec_first = 0, num = 0;             // records [rec_first, rec_first + num)
  uint64_t lo = 0, hi = 0;
  size_t dev_first = 0, dev_end = 0;         // device blocks [dev_first, dev_end)
  size_t n_edges = 0, edge[2] = {0, 0}, cbeg = 0, cend = 0;
  size_t dev_blocks() const { return dev_end - dev_first; }
};
int32_t plan_shard(const BgzfIndex& idx, size_t shard, size_t n_shards, ShardPlan* plan);
// The same plan for records [rec_first, rec_first + num) (plan_shard is this over ibu_shard_range, with the whole file crossing the link
// when there is one shard): only the device blocks' bytes cross the link.
int32_t plan_records(const BgzfIndex& idx, size_t rec_first, size_t num, ShardPlan* plan);
// The records of every range but the last of the pull stream over the file (ibu_stream_open_path): about `target_bytes` compressed bytes
// at the file's ratio, a multiple of the reference's refill (IBU_DEFAULT_BUFFER_SIZE: 49 152 records), and of lcm(slot_records, 49 152)
// where that is no larger — every batch but the last is then a whole slot: the multiple nearest the target, at least one; a target of the
// whole file or more is one range.  The ranges: ceil(records / this).
size_t plan_range_records(const BgzfIndex& idx, size_t target_bytes, size_t slot_records);

}  // namespace ibu
