// bgzf_plan.cpp — the walk over a BGZF file's block headers, the host inflate of single blocks, and the plan of one shard.
#include "bgzf_plan.hpp"

#include <algorithm>

#include "common.hpp"

namespace ibu {
namespace {

// The walk, in pieces side by side.  A block's start cannot be computed without the blocks in front of it, but it can be GUESSED: every
// piece but the first looks for the 16 bytes a bgzip header begins with (1f 8b 08 04 .. 06 00 'B' 'C' 02 00) at or behind its first
// byte and walks the chain from there to the end of its piece.  The guesses are then checked: piece i's chain must END exactly where
// piece i + 1's began — where it does not (the signature inside compressed data, an unusual extra field), or anything at all is off,
// the plain walk from byte 0 decides, errors included.  (184 k blocks of a 6 GB file: 60 ms of page faults in one thread.)
bool walk_pieces(const uint8_t* map, size_t size, BgzfIndex* idx) {
  const size_t T = 8;
  struct Piece { size_t begin = 0, end = 0; bool ok = false; uint64_t out = 0; std::vector<ibu_inflate_block_t> blocks; };
  std::vector<Piece> pc(T);
  auto run = [&](size_t i) {
    Piece& P = pc[i];
    try {
      const size_t lo = size / T * i, hi = i + 1 == T ? size : size / T * (i + 1);
      size_t pos = lo;
      if (i) {                                           // the first header-like spot at or behind lo
        const uint8_t sig_a[4] = {0x1f, 0x8b, 0x08, 0x04}, sig_b[6] = {0x06, 0x00, 'B', 'C', 0x02, 0x00};
        for (;; ++pos) {
          if (pos + 18 > size || pos >= hi) return;      // none in this piece: give up (the plain walk decides)
          if (memcmp(map + pos, sig_a, 4) == 0 && memcmp(map + pos + 10, sig_b, 6) == 0) break;
        }
      }
      P.begin = pos;
      std::vector<ibu_inflate_block_t> part(1 << 14);
      while (pos < hi) {
        size_t nb = 0, consumed = 0, cap = part.size();
        uint64_t ob = 0;
        if (ibu_bgzf_scan(map + pos, size - pos, 1, part.data(), cap, &nb, &consumed, &ob) != IBU_OK || consumed == 0) return;
        size_t keep = 0, bytes = 0;                      // only the blocks that START inside the piece
        uint64_t outb = 0;
        for (; keep < nb; ++keep) {
          const size_t start = pos + (size_t)part[keep].comp_offset - 18;   // (bgzip's header: 18 bytes; checked again when the pieces are joined)
          if (start >= hi) break;
          bytes = (size_t)part[keep].comp_offset + part[keep].comp_len + 8;
          part[keep].comp_offset += pos;
          part[keep].out_offset += (int64_t)P.out;
          outb = (uint64_t)(part[keep].out_offset - (int64_t)P.out) + part[keep].out_len;
        }
        P.blocks.insert(P.blocks.end(), part.begin(), part.begin() + (ptrdiff_t)keep);
        P.out += outb;
        pos += bytes;
        if (keep < nb || keep == 0) break;
      }
      P.end = pos;
      P.ok = true;
    } catch (...) {}
  };
  run_pieces((unsigned)T, run);
  size_t nblocks = 0;
  for (size_t i = 0; i < T; ++i) {
    if (!pc[i].ok || (i == 0 && pc[i].begin != 0) || (i && pc[i].begin != pc[i - 1].end)) return false;
    nblocks += pc[i].blocks.size();
  }
  if (pc[T - 1].end != size) return false;
  idx->blocks.reserve(nblocks);
  for (size_t i = 0; i < T; ++i) {
    for (ibu_inflate_block_t& b : pc[i].blocks) b.out_offset += (int64_t)idx->total;
    idx->blocks.insert(idx->blocks.end(), pc[i].blocks.begin(), pc[i].blocks.end());
    idx->total += pc[i].out;
  }
  return true;
}

}  // namespace

int32_t inflate_block_on_host(pgz::RawInflater& raw, const uint8_t* map, const ibu_inflate_block_t& b, uint8_t* out) {
  std::vector<uint8_t> in(map + b.comp_offset, map + b.comp_offset + b.comp_len);
  in.resize(b.comp_len + 512, 0);                        // the decoder may read (not use) a few bytes behind the stream
  uint32_t crc = 0;
  const int e = raw.inflate(in.data(), b.comp_len, out, b.out_len, &crc);
  if (e == ENOMEM) return err_io(ENOMEM, "inflate");
  if (e || crc != b.crc32) return err_niffler("a BGZF block does not inflate to its announced length and CRC-32");
  return IBU_OK;
}

int32_t bgzf_index(const uint8_t* map, size_t size, BgzfIndex* idx, size_t pieces_min_bytes) try {
  *idx = BgzfIndex();
  idx->file_bytes = size;
  std::vector<ibu_inflate_block_t>& B = idx->blocks;
  bool have = false;
  try { have = size >= pieces_min_bytes && walk_pieces(map, size, idx); } catch (...) {}
  if (!have) { B.clear(); idx->total = 0; }
  idx->in_pieces = have;
  std::vector<ibu_inflate_block_t> part(have ? 1 : 1 << 16);
  for (size_t pos = have ? size : 0; pos < size;) {      // 1. the blocks (a cut-off or foreign member: IBU_ERR_NIFFLER from the walk)
    size_t nb = 0, consumed = 0;
    uint64_t ob = 0;
    const int32_t rc = ibu_bgzf_scan(map + pos, size - pos, 1, part.data(), part.size(), &nb, &consumed, &ob);
    for (size_t i = 0; i < nb; ++i) {
      part[i].comp_offset += pos;
      part[i].out_offset += (int64_t)idx->total;
    }
    B.insert(B.end(), part.begin(), part.begin() + (ptrdiff_t)nb);
    if (rc) return rc;
    if (consumed == 0) return err_niffler("the stream ends inside a BGZF block");
    pos += consumed;
    idx->total += ob;
  }
  pgz::RawInflater raw;                                  // 2. the header: the leading blocks, inflated here
  std::vector<uint8_t> head(IBU_HEADER_SIZE + 65536);
  size_t lead_bytes = 0;
  while (lead_bytes < IBU_HEADER_SIZE && idx->lead < B.size()) {   // (an empty block, too: "01 00" is refused as the Reader refuses it)
    const ibu_inflate_block_t& b = B[idx->lead++];
    if (int32_t rc = inflate_block_on_host(raw, map, b, head.data() + lead_bytes)) return rc;
    lead_bytes += b.out_len;
  }
  if (lead_bytes < IBU_HEADER_SIZE) return err_io(0, "read header");
  idx->head.assign(head.begin(), head.begin() + (ptrdiff_t)lead_bytes);
  memcpy(&idx->header, head.data(), IBU_HEADER_SIZE);
  if (int32_t rc = ibu_header_validate(&idx->header)) return rc;
  return (idx->total - IBU_HEADER_SIZE) % IBU_RECORD_SIZE ? err_map_size() : IBU_OK;
} catch (...) {
  return caught_io("ibu_load_bgzf_to_device");
}

int32_t plan_shard(const BgzfIndex& idx, size_t shard, size_t n_shards, ShardPlan* plan) {
  size_t rs = 0, re = 0;
  if (int32_t rc = ibu_shard_range((size_t)((idx.total - IBU_HEADER_SIZE) / IBU_RECORD_SIZE), n_shards, shard, &rs, &re)) return rc;
  const int32_t rc = plan_records(idx, rs, re - rs, plan);
  if (rc == IBU_OK && n_shards == 1) {                     // all of the file: the copies can start before the walk is done
    plan->cbeg = 0;
    plan->cend = idx.file_bytes;
  }
  return rc;
}

int32_t plan_records(const BgzfIndex& idx, size_t rec_first, size_t num, ShardPlan* plan) {
  ShardPlan& p = *plan = ShardPlan();
  const std::vector<ibu_inflate_block_t>& B = idx.blocks;
  if (rec_first + num < rec_first || rec_first + num > (size_t)((idx.total - IBU_HEADER_SIZE) / IBU_RECORD_SIZE)) return err_arg("records out of range");
  p.rec_first = rec_first;
  p.num = num;
  p.lo = IBU_HEADER_SIZE + (uint64_t)IBU_RECORD_SIZE * rec_first;
  p.hi = IBU_HEADER_SIZE + (uint64_t)IBU_RECORD_SIZE * (rec_first + num);
  p.dev_first = idx.lead;
  while (p.dev_first < B.size() && (uint64_t)B[p.dev_first].out_offset < p.lo) ++p.dev_first;
  p.dev_end = p.dev_first;
  while (p.dev_end < B.size() && (uint64_t)B[p.dev_end].out_offset + B[p.dev_end].out_len <= p.hi) ++p.dev_end;
  const size_t straddle[2] = {p.dev_first > idx.lead ? p.dev_first - 1 : B.size(), p.dev_end};   // the blocks around lo / hi
  for (size_t i : straddle) {
    if (p.num && i < B.size() && B[i].out_len && (uint64_t)B[i].out_offset < p.hi && (uint64_t)B[i].out_offset + B[i].out_len > p.lo)
      p.edge[p.n_edges++] = i;
  }
  if (p.dev_blocks()) {                                    // only the device blocks' bytes cross the link
    p.cbeg = (size_t)B[p.dev_first].comp_offset;
    p.cend = (size_t)(B[p.dev_end - 1].comp_offset + B[p.dev_end - 1].comp_len);
  }
  return IBU_OK;
}

size_t plan_range_records(const BgzfIndex& idx, size_t target_bytes, size_t slot_records) {
  const size_t refill = IBU_DEFAULT_BUFFER_SIZE / IBU_RECORD_SIZE;
  const size_t n = (size_t)((idx.total - IBU_HEADER_SIZE) / IBU_RECORD_SIZE);
  const size_t per = target_bytes >= idx.file_bytes ? n : (size_t)((double)n * (double)target_bytes / (double)(idx.file_bytes ? idx.file_bytes : 1));
  size_t unit = refill;
  if (slot_records) {
    size_t a = slot_records, b = refill;                   // gcd
    while (b) { const size_t t = a % b; a = b; b = t; }
    const size_t lcm = slot_records / a * refill;
    if (lcm <= per) unit = lcm;
  }
  if (per >= n) return std::max((n + unit - 1) / unit, (size_t)1) * unit;   // one range
  return std::max((per + unit / 2) / unit, (size_t)1) * unit;
}

}  // namespace ibu
