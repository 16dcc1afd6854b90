// api_records.cpp — the entry points of the C ABI (include/ibu_hip.h) that work on records and their columns: the codecs, reduce,
// generate, copy and compare, the compacted keys, the device inflate, sort and merge.  The context itself: device.cpp.
#include <stddef.h>

#include <utility>
#include <vector>

#include "ctx.hpp"

using namespace ibu;

// ---- K1 / K1' ------------------------------------------------------------------------------
extern "C" int32_t ibu_deserialize(ibu_ctx_t* ctx, const void* d_records, size_t n, uint64_t* d_barcode,
                                   uint64_t* d_umi, uint64_t* d_index, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !d_barcode || !d_umi || !d_index) return err_arg("NULL device pointer");
  if (!aligned8(d_records) || !aligned8(d_barcode) || !aligned8(d_umi) || !aligned8(d_index))
    return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_deserialize(ctx->cfg, d_records, n, d_barcode, d_umi, d_index, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_serialize(ibu_ctx_t* ctx, const uint64_t* d_barcode, const uint64_t* d_umi,
                                 const uint64_t* d_index, size_t n, void* d_records, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !d_barcode || !d_umi || !d_index) return err_arg("NULL device pointer");
  if (!aligned8(d_records) || !aligned8(d_barcode) || !aligned8(d_umi) || !aligned8(d_index))
    return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_serialize(ctx->cfg, d_barcode, d_umi, d_index, n, d_records, pick_stream(ctx, stream)));
  return IBU_OK;
}

// ---- column codec ----------------------------------------------------------------------------
extern "C" int32_t ibu_unpack_2bit(ibu_ctx_t* ctx, const uint64_t* d_codes, size_t n, uint32_t len, uint8_t* d_ascii,
                                   void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (len == 0 || len > 32) return err_seq_len(len);
  if (n == 0) return IBU_OK;
  if (!d_codes || !d_ascii) return err_arg("NULL device pointer");
  if (!aligned8(d_codes)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_unpack(ctx->cfg, d_codes, n, len, d_ascii, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_pack_2bit(ibu_ctx_t* ctx, const uint8_t* d_ascii, size_t n, uint32_t len, uint64_t* d_codes,
                                 void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (len == 0 || len > 32) return err_seq_len(len);
  if (n == 0) return IBU_OK;
  if (!d_codes || !d_ascii) return err_arg("NULL device pointer");
  if (!aligned8(d_codes)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_pack(ctx->cfg, d_ascii, n, len, d_codes, ctx->d_status, pick_stream(ctx, stream)));
  return IBU_OK;
}

// ---- K2 / K3 -----------------------------------------------------------------------------------
extern "C" int32_t ibu_decode_ascii(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t bc_len, uint32_t umi_len,
                                    uint8_t* d_bc_ascii, uint8_t* d_umi_ascii, uint64_t* d_index, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_lens(bc_len, umi_len)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records) return err_arg("d_records is NULL");
  if (!aligned8(d_records) || !aligned8(d_index)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_decode(ctx->cfg, d_records, n, bc_len, umi_len, d_bc_ascii, d_umi_ascii, d_index,
                        pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_encode_ascii(ibu_ctx_t* ctx, const uint8_t* d_bc_ascii, const uint8_t* d_umi_ascii,
                                    const uint64_t* d_index, uint64_t first_index, size_t n, uint32_t bc_len,
                                    uint32_t umi_len, void* d_records, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_lens(bc_len, umi_len)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !d_bc_ascii || !d_umi_ascii) return err_arg("NULL device pointer");
  if (!aligned8(d_records) || !aligned8(d_index)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_encode(ctx->cfg, d_bc_ascii, d_umi_ascii, d_index, first_index, n, bc_len, umi_len, d_records,
                        ctx->d_status, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_codec_status(ibu_ctx_t* ctx, void* stream, uint64_t* first_bad_record, uint64_t* n_bad_records) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  IBU_HIP(read_back<2>(ctx, ctx->d_status, st));
  const uint64_t first = ctx->h_pinned[0], nbad = ctx->h_pinned[1];
  if (first_bad_record) *first_bad_record = first;
  if (n_bad_records) *n_bad_records = nbad;
  if (nbad == 0) return IBU_OK;
  IBU_HIP(launch_fill2(ctx->d_status, ~0ull, 0, st));  // re-arm
  return set_error(IBU_ERR_INVALID_BASE, first, nbad, 0,
                   "Invalid base: %llu record(s) hold a byte outside ACGTacgt, first at record %llu",
                   (unsigned long long)nbad, (unsigned long long)first);
}

// ---- K4 ---------------------------------------------------------------------------------------------
extern "C" int32_t ibu_reduce_reset(ibu_ctx_t* ctx, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  IBU_HIP(hipMemsetAsync(ctx->d_acc, 0, kReduceAccBytes, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_reduce(ibu_ctx_t* ctx, const void* d_records, size_t n, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  IBU_HIP(launch_reduce(ctx->cfg, d_records, n, ctx->d_acc, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_reduce_fetch(ibu_ctx_t* ctx, void* stream, ibu_reduce_result_t* out) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  hipStream_t st = pick_stream(ctx, stream);
  IBU_HIP(launch_reduce_fold(ctx->d_acc, st));
  IBU_HIP(read_back<8>(ctx, ctx->d_acc, st));
  out->count = ctx->h_pinned[0];
  for (int k = 0; k < 3; ++k) {
    out->sum[k] = ctx->h_pinned[1 + k];
    out->xor_[k] = ctx->h_pinned[4 + k];
  }
  return IBU_OK;
}

// ---- synthetic records, sortedness, sort ---------------------------------------------------------------
extern "C" int32_t ibu_generate(ibu_ctx_t* ctx, uint64_t seed, uint64_t first, size_t n, uint32_t bc_len,
                                uint32_t umi_len, void* d_records, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_lens(bc_len, umi_len)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  IBU_HIP(launch_generate(ctx->cfg, seed, first, n, bc_len, umi_len, d_records, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_device_copy(ibu_ctx_t* ctx, void* d_dst, const void* d_src, size_t bytes, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (bytes == 0) return IBU_OK;
  if (!d_dst || !d_src) return err_arg("NULL device pointer");
  if (ranges_overlap(d_dst, bytes, d_src, bytes)) return err_arg("source and destination overlap");
  IBU_HIP(launch_copy(ctx->cfg, d_src, d_dst, bytes, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_lower_bound_records(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, const void* d_keys, size_t k,
                                           uint64_t* d_pos, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (k == 0) return IBU_OK;
  if (k > (1u << 20)) return err_arg("at most 2^20 keys per call");
  if ((rc = check_u64_ptrs({d_keys, d_pos}, "d_keys / d_pos")) != 0) return rc;
  if (n && (rc = check_u64_ptr(d_sorted_records, "d_sorted_records")) != 0) return rc;
  IBU_HIP(launch_lower_bound(d_sorted_records, n, d_keys, k, d_pos, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_is_sorted(ibu_ctx_t* ctx, const void* d_records, size_t n, void* stream, int32_t* sorted) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!sorted) return err_arg("sorted is NULL");
  *sorted = 1;
  if (n < 2) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  IBU_HIP(hipMemsetAsync(ctx->d_flag, 0, 4, st));
  IBU_HIP(launch_sorted_check(ctx->cfg, d_records, n, ctx->d_flag, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned + 8, ctx->d_flag, 4, hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  *sorted = (*reinterpret_cast<uint32_t*>(ctx->h_pinned + 8)) == 0;
  return IBU_OK;
}
// `a == b` on two device-resident record slices, with the position (Record: PartialEq / Eq, record.rs:58).
extern "C" int32_t ibu_records_first_mismatch(ibu_ctx_t* ctx, const void* d_a, const void* d_b, size_t n, uint64_t* first,
                                              void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!first) return err_arg("first is NULL");
  *first = n;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptrs({d_a, d_b}, "d_a / d_b")) != 0) return rc;
  if (n > (~(size_t)0) / 3) return err_arg("n too large");
  hipStream_t st = pick_stream(ctx, stream);
  uint64_t* slot = reinterpret_cast<uint64_t*>(ctx->d_flag) + 1;   // d_flag: 16 bytes; [0] is the sortedness flag
  IBU_HIP(hipMemsetAsync(slot, 0xFF, 8, st));
  IBU_HIP(launch_mismatch(ctx->cfg, d_a, d_b, 3 * n, slot, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned + 10, slot, 8, hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  const uint64_t w = ctx->h_pinned[10];
  if (w != ~0ull) *first = w / 3;
  return IBU_OK;
}
// ---- compacted keys: census, plan, records <-> 12-byte elements (the exchange format of the multi-GPU sort) ----------
static_assert(sizeof(ibu_key_plan_t) == sizeof(ibu::CompactPlan) && offsetof(ibu_key_plan_t, base) == offsetof(ibu::CompactPlan, base) &&
                  offsetof(ibu_key_plan_t, k) == offsetof(ibu::CompactPlan, k),
              "ibu_key_plan_t is the kernels' CompactPlan");
static_assert(sizeof(ibu_inflate_block_t) == sizeof(InflateBlockDesc) && offsetof(ibu_inflate_block_t, crc32) == offsetof(InflateBlockDesc, crc) &&
              offsetof(ibu_inflate_block_t, out_offset) == offsetof(InflateBlockDesc, ooff) && IBU_INFLATE_PAD == kInflatePad,
              "ibu_inflate_block_t is the kernel's descriptor");
extern "C" int32_t ibu_inflate_blocks_device(ibu_ctx_t* ctx, const void* d_comp, const ibu_inflate_block_t* d_blocks, size_t n, void* d_out,
                                             uint32_t* d_status, uint32_t* d_first_bad, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_comp || !d_blocks || !d_out || !d_status || !d_first_bad) return err_arg("NULL argument");
  if (n >= (1ull << 31)) return err_arg("fewer than 2^31 blocks per call");
  rc = ensure_sort_scratch(ctx, inflate_scratch_bytes(ctx->cfg, n));   // (the lanes' symbol tables: the context's scratch, as the sort's)
  if (rc) return rc;
  IBU_HIP(launch_inflate_blocks(ctx->cfg, d_comp, reinterpret_cast<const InflateBlockDesc*>(d_blocks), n, d_out, d_status, d_first_bad,
                                ctx->d_sort_scratch, ctx->sort_scratch_bytes, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_records_census(ibu_ctx_t* ctx, const void* d_records, size_t n, uint64_t out[8], void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  if (n && (rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  rc = ensure_sort_scratch(ctx, 4096);   // the census slots (sort.hip: kCensusBytes)
  if (rc) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  uint64_t* d_c = static_cast<uint64_t*>(ctx->d_sort_scratch);
  IBU_HIP(launch_records_census(ctx->cfg, d_records, n, d_c, st));
  IBU_HIP(hipMemcpyAsync(out, d_c, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  return IBU_OK;
}
extern "C" int32_t ibu_key_plan_init(const uint64_t or_words[3], const uint64_t and_words[3], ibu_key_plan_t* plan) {
  if (!or_words || !and_words || !plan) return err_arg("NULL argument");
  compact_plan_init(or_words, and_words, reinterpret_cast<CompactPlan*>(plan));
  return IBU_OK;
}
static int32_t check_plan(const ibu_key_plan_t* plan) {
  if (!plan) return err_arg("plan is NULL");
  if (plan->k > 12) return err_arg("more than 12 key bytes vary: these records do not fit 12-byte elements");
  return IBU_OK;
}
extern "C" int32_t ibu_records_compact(ibu_ctx_t* ctx, const ibu_key_plan_t* plan, const void* d_records, size_t n, void* d_elems,
                                       void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_plan(plan)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if (!d_elems || (reinterpret_cast<uintptr_t>(d_elems) & 3u)) return err_arg("d_elems must be non-NULL and 4-byte aligned");
  IBU_HIP(launch_compact(ctx->cfg, *reinterpret_cast<const CompactPlan*>(plan), d_records, n, d_elems, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_records_expand(ibu_ctx_t* ctx, const ibu_key_plan_t* plan, const void* d_elems, size_t n, void* d_records,
                                      void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_plan(plan)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if (!d_elems || (reinterpret_cast<uintptr_t>(d_elems) & 3u)) return err_arg("d_elems must be non-NULL and 4-byte aligned");
  IBU_HIP(launch_expand(ctx->cfg, *reinterpret_cast<const CompactPlan*>(plan), d_elems, n, d_records, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_sort_records(ibu_ctx_t* ctx, void* d_records, void* d_tmp, size_t n, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n < 2) return IBU_OK;
  if ((rc = check_u64_ptrs({d_records, d_tmp}, "d_records / d_tmp")) != 0) return rc;
  if ((rc = check_below_2_40(n, "sort_records", "records")) != 0) return rc;
  rc = ensure_sort_scratch(ctx, sort_scratch_bytes(ctx->cfg, n));
  if (rc) return rc;
  IBU_HIP(launch_sort_records(ctx->cfg, d_records, d_tmp, n, ctx->d_sort_scratch, ctx->sort_scratch_bytes,
                              pick_stream(ctx, stream)));
  return IBU_OK;
}
// ---- merge of sorted records (k_merge.hip).  The semantics are this library's: include/ibu_hip.h.
// One two-way merge, arguments checked by the caller; an empty input is a copy of the other (and its source bytes a fill).
static int32_t merge_two(ibu_ctx_t* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, uint8_t* d_source, hipStream_t st) {
  if (na == 0 || nb == 0) {
    const size_t n = na + nb;
    if (n == 0) return IBU_OK;
    IBU_HIP(launch_copy(ctx->cfg, na ? d_a : d_b, d_out, 24 * n, st));
    if (d_source) IBU_HIP(hipMemsetAsync(d_source, na ? 0 : 1, n, st));
    return IBU_OK;
  }
  IBU_HIP(launch_merge(ctx->cfg, d_a, na, d_b, nb, d_out, d_source, ctx->d_sort_scratch, st));
  return IBU_OK;
}
extern "C" int32_t ibu_merge_sorted(ibu_ctx_t* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, uint8_t* d_source,
                                    void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (na >= (1ull << 40) || nb >= (1ull << 40)) return err_arg("merge_sorted handles fewer than 2^40 records per input");
  const size_t n = na + nb;
  if (n == 0) return IBU_OK;
  if ((na && (!d_a || !aligned8(d_a))) || (nb && (!d_b || !aligned8(d_b))) || !d_out || !aligned8(d_out))
    return err_arg("d_a / d_b / d_out must be non-NULL and 8-byte aligned");
  if (ranges_overlap(d_out, 24 * n, d_a, 24 * na) || ranges_overlap(d_out, 24 * n, d_b, 24 * nb)) return err_arg("d_out overlaps an input");
  rc = ensure_sort_scratch(ctx, merge_scratch_bytes(n));
  if (rc) return rc;
  return merge_two(ctx, d_a, na, d_b, nb, d_out, d_source, pick_stream(ctx, stream));
}
extern "C" int32_t ibu_merge_sorted_runs(ibu_ctx_t* ctx, void* d_records, void* d_tmp, const size_t* run_lengths, size_t k, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (k == 0) return IBU_OK;
  if (!run_lengths) return err_arg("run_lengths is NULL");
  size_t n = 0;
  for (size_t i = 0; i < k; ++i) {
    if ((rc = check_below_2_40(run_lengths[i], "merge_sorted_runs", "records")) != 0) return rc;
    n += run_lengths[i];
    if ((rc = check_below_2_40(n, "merge_sorted_runs", "records")) != 0) return rc;
  }
  if (n == 0 || k == 1) return IBU_OK;
  if ((rc = check_u64_ptrs({d_records, d_tmp}, "d_records / d_tmp")) != 0) return rc;
  if (ranges_overlap(d_records, 24 * n, d_tmp, 24 * n)) return err_arg("d_tmp overlaps d_records");
  rc = ensure_sort_scratch(ctx, merge_scratch_bytes(n));   // once, for the largest merge: nothing is allocated between the levels
  if (rc) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  std::vector<size_t> runs(run_lengths, run_lengths + k), next;
  uint8_t* from = static_cast<uint8_t*>(d_records);
  uint8_t* to = static_cast<uint8_t*>(d_tmp);
  while (runs.size() > 1) {                                // one level: neighbouring runs pairwise, an unpaired last run copied
    next.clear();
    size_t at = 0;
    for (size_t i = 0; i < runs.size(); i += 2) {
      const size_t na = runs[i], nb = i + 1 < runs.size() ? runs[i + 1] : 0;
      rc = merge_two(ctx, from + 24 * at, na, from + 24 * (at + na), nb, to + 24 * at, nullptr, st);
      if (rc) return rc;
      next.push_back(na + nb);
      at += na + nb;
    }
    runs.swap(next);
    std::swap(from, to);
  }
  if (from != d_records) IBU_HIP(launch_copy(ctx->cfg, from, d_records, 24 * n, st));   // an odd number of levels ended in d_tmp
  return IBU_OK;
}
