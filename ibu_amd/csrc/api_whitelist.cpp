// api_whitelist.cpp — the entry points of the C ABI (include/ibu_hip.h) around a barcode whitelist: the table, correction, the
// abundance counters and the resolution of ambiguous barcodes, the per-barcode labels, and the selection of records by class
// (k_whitelist.hip).
#include <string.h>

#include <atomic>

#include "ctx.hpp"
#include "partition_plan.hpp"

using namespace ibu;

// ---- barcode correction against a whitelist (k_whitelist.hip) --------------------------------------------------------
struct ibu_whitelist {
  ibu_ctx* ctx = nullptr;
  void* d_mem = nullptr;       // the table's slots, then the build's four status words
  size_t slots = 0, n_distinct = 0, device_bytes = 0;
  uint32_t bc_len = 0;
  bool has_ones = false;       // the all-ones key (a legal code at 32 bases only) is in the whitelist
};
static WhitelistTable table_of(const ibu_whitelist* wl) {
  return WhitelistTable{static_cast<const uint64_t*>(wl->d_mem), wl->slots, wl->bc_len, wl->has_ones};
}
// A *_create call without a context has nothing to build on: say whether a device is missing altogether.  what: "a whitelist".
static int32_t no_ctx_error(const char* what) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  if (count == 0) return set_error(IBU_ERR_NO_DEVICE, 0, 0, 0, "no HIP device: %s lives on a device context", what);
  return err_arg("ctx is NULL");
}
extern "C" int32_t ibu_whitelist_create(ibu_ctx_t* ctx, const uint64_t* d_codes, size_t w, uint32_t bc_len, void* stream,
                                        ibu_whitelist_t** out) {
  if (!ctx) return no_ctx_error("a whitelist");
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  *out = nullptr;
  if (w == 0) return err_arg("a whitelist needs at least one code");
  if (bc_len == 0 || bc_len > 32) return err_arg("bc_len must be 1..32");
  if ((rc = check_u64_ptr(d_codes, "d_codes")) != 0) return rc;
  if (w > (1ull << 31)) return err_arg("a whitelist holds at most 2^31 codes");
  hipStream_t st = pick_stream(ctx, stream);
  ibu_whitelist* wl = new ibu_whitelist;
  wl->ctx = ctx;
  wl->bc_len = bc_len;
  wl->slots = whitelist_slots(w);
  wl->device_bytes = wl->slots * sizeof(uint64_t) + 4 * sizeof(uint64_t);
  hipError_t e = ctx_malloc(ctx, &wl->d_mem, wl->device_bytes);
  uint64_t* table = static_cast<uint64_t*>(wl->d_mem);
  uint64_t* status = table ? table + wl->slots : nullptr;
  if (e == hipSuccess) e = hipMemsetAsync(table, 0xFF, (wl->slots + 1) * sizeof(uint64_t), st);   // free slots, status[0] = no bad code
  if (e == hipSuccess) e = hipMemsetAsync(status + 1, 0, 3 * sizeof(uint64_t), st);
  if (e == hipSuccess) e = launch_whitelist_build(ctx->cfg, d_codes, w, bc_len, table, wl->slots, status, st);
  if (e == hipSuccess) e = read_back<4>(ctx, status, st);
  if (e != hipSuccess) {
    ibu_whitelist_destroy(wl);
    return hip_fail(e, "ibu_whitelist_create");
  }
  const uint64_t first_bad = ctx->h_pinned[0];
  wl->n_distinct = ctx->h_pinned[1];
  wl->has_ones = ctx->h_pinned[2] != 0;
  if (first_bad != ~0ull) {
    ibu_whitelist_destroy(wl);
    return set_error(IBU_ERR_INVALID_ARG, first_bad, bc_len, 0, "Invalid argument: whitelist code %llu has bits at or above 2*bc_len (bc_len %u)",
                     (unsigned long long)first_bad, bc_len);
  }
  *out = wl;
  return IBU_OK;
}
extern "C" int32_t ibu_whitelist_info(const ibu_whitelist_t* wl, uint32_t* bc_len, size_t* n_distinct, size_t* device_bytes) {
  if (!wl) return err_arg("wl is NULL");
  if (bc_len) *bc_len = wl->bc_len;
  if (n_distinct) *n_distinct = wl->n_distinct;
  if (device_bytes) *device_bytes = wl->device_bytes;
  return IBU_OK;
}
extern "C" void ibu_whitelist_destroy(ibu_whitelist_t* wl) {
  if (!wl) return;
  if (wl->d_mem) {
    (void)hipSetDevice(wl->ctx->device);
    (void)hipFree(wl->d_mem);   // (waits for launches that still probe the table)
  }
  delete wl;
}
extern "C" int32_t ibu_correct_barcodes(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, void* d_records, size_t n, uint32_t max_mismatches,
                                        uint8_t* d_class, ibu_correct_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  if (max_mismatches > 1) return err_arg("max_mismatches must be 0 or 1");
  if (counts) *counts = ibu_correct_counts_t{0, 0, 0, 0};
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "correct_barcodes", "records")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  const auto correct = [&](uint64_t* acc) { return launch_correct(ctx->cfg, table_of(wl), d_records, n, max_mismatches, d_class, acc, st); };
  if (!counts) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(correct(nullptr));
    return IBU_OK;
  }
  if ((rc = grid_totals<4>(ctx, st, correct)) != 0) return rc;
  counts->exact = ctx->h_pinned[0];
  counts->corrected = ctx->h_pinned[1];
  counts->ambiguous = ctx->h_pinned[2];
  counts->unmatched = ctx->h_pinned[3];
  return IBU_OK;
}
// ---- whitelist abundance and the resolution of ambiguous barcodes (k_whitelist.hip) ----------------------------------------
struct ibu_abundance {
  ibu_ctx* ctx = nullptr;
  const ibu_whitelist* wl = nullptr;
  uint64_t* d_counters = nullptr;          // slots + 1: one per table slot, the last for the all-ones key
  size_t device_bytes = 0;
  std::atomic<uint64_t> offered{0};        // records offered to ibu_abundance_add since create / reset: no counter can pass it
};
static constexpr uint64_t kAbundanceMax = 1ull << 40;
extern "C" int32_t ibu_abundance_create(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, void* stream, ibu_abundance_t** out) {
  if (!ctx) return no_ctx_error("an abundance");
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  *out = nullptr;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  hipStream_t st = pick_stream(ctx, stream);
  ibu_abundance* ab = new ibu_abundance;
  ab->ctx = ctx;
  ab->wl = wl;
  ab->device_bytes = (wl->slots + 1) * sizeof(uint64_t);
  hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&ab->d_counters), ab->device_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(ab->d_counters, 0, ab->device_bytes, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    ibu_abundance_destroy(ab);
    return hip_fail(e, "ibu_abundance_create");
  }
  *out = ab;
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_reset(ibu_abundance_t* ab, void* stream) {
  if (!ab) return err_arg("ab is NULL");
  int32_t rc = check_ctx(ab->ctx);
  if (rc) return rc;
  IBU_HIP(hipMemsetAsync(ab->d_counters, 0, ab->device_bytes, pick_stream(ab->ctx, stream)));
  ab->offered.store(0);
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_info(const ibu_abundance_t* ab, size_t* device_bytes) {
  if (!ab) return err_arg("ab is NULL");
  if (device_bytes) *device_bytes = ab->device_bytes;
  return IBU_OK;
}
extern "C" void ibu_abundance_destroy(ibu_abundance_t* ab) {
  if (!ab) return;
  if (ab->d_counters) {
    (void)hipSetDevice(ab->ctx->device);
    (void)hipFree(ab->d_counters);   // (waits for launches that still add to or read the counters)
  }
  delete ab;
}
static int32_t check_abundance(const ibu_ctx* ctx, const ibu_abundance* ab) {
  if (!ab) return err_arg("ab is NULL");
  if (ab->ctx != ctx) return err_arg("the abundance was created on another context");
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_add(ibu_ctx_t* ctx, ibu_abundance_t* ab, const void* d_records, const uint8_t* d_class, size_t n,
                                     uint32_t class_mask, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_abundance(ctx, ab)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "abundance_add", "records")) != 0) return rc;
  uint64_t seen = ab->offered.load();
  do {
    if (seen + n > kAbundanceMax)
      return set_error(IBU_ERR_INVALID_ARG, seen, n, 0, "Invalid argument: %llu records offered so far and %llu more would pass 2^40 (reset the abundance)",
                       (unsigned long long)seen, (unsigned long long)n);
  } while (!ab->offered.compare_exchange_weak(seen, seen + n));
  IBU_HIP(launch_abundance_add(ctx->cfg, table_of(ab->wl), d_records, d_class, n, class_mask & 0xFFu, ab->d_counters, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_counts(ibu_ctx_t* ctx, const ibu_abundance_t* ab, const uint64_t* d_codes, size_t k, uint64_t* d_counts,
                                        void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_abundance(ctx, ab)) != 0) return rc;
  if (k == 0) return IBU_OK;
  if ((rc = check_u64_ptrs({d_codes, d_counts}, "d_codes / d_counts")) != 0) return rc;
  if ((rc = check_below_2_40(k, "abundance_counts", "codes")) != 0) return rc;
  IBU_HIP(launch_abundance_counts(ctx->cfg, table_of(ab->wl), ab->d_counters, d_codes, k, d_counts, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_resolve_barcodes(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, const ibu_abundance_t* ab, void* d_records, size_t n,
                                        uint64_t num, uint64_t den, uint8_t* d_class, ibu_resolve_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  if ((rc = check_abundance(ctx, ab)) != 0) return rc;
  if (ab->wl != wl) return err_arg("the abundance belongs to another whitelist");
  if (num < 1 || num > den || den >= (1ull << 24) || 2 * num <= den)
    return err_arg("the share num / den must satisfy 1 <= num <= den < 2^24 and 2 * num > den");
  if (counts) *counts = ibu_resolve_counts_t{0, 0, 0, 0};
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if (!d_class) return err_arg("d_class is NULL");
  if ((rc = check_below_2_40(n, "resolve_barcodes", "records")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  const auto resolve = [&](uint64_t* acc) { return launch_resolve(ctx->cfg, table_of(wl), ab->d_counters, d_records, n, num, den, d_class, acc, st); };
  if (!counts) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(resolve(nullptr));
    return IBU_OK;
  }
  if ((rc = grid_totals<4>(ctx, st, resolve)) != 0) return rc;
  counts->examined = ctx->h_pinned[0];
  counts->resolved = ctx->h_pinned[1];
  counts->below_share = ctx->h_pinned[2];
  counts->unseen = ctx->h_pinned[3];
  return IBU_OK;
}
// ---- per-barcode labels onto records (k_whitelist.hip) --------------------------------------------------------------------
struct ibu_labels {
  ibu_ctx* ctx = nullptr;
  const ibu_whitelist* wl = nullptr;
  uint8_t* d_labels = nullptr;             // slots + 1: one per table slot, the last for the all-ones key
  size_t device_bytes = 0;
};
static int32_t check_labels(const ibu_ctx* ctx, const ibu_labels* lb) {
  if (!lb) return err_arg("lb is NULL");
  if (lb->ctx != ctx) return err_arg("the labels were created on another context");
  return IBU_OK;
}
extern "C" int32_t ibu_labels_create(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, uint32_t fill, void* stream, ibu_labels_t** out) {
  if (!ctx) return no_ctx_error("a label table");
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  *out = nullptr;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  if ((rc = check_byte(fill, "fill")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  ibu_labels* lb = new ibu_labels;
  lb->ctx = ctx;
  lb->wl = wl;
  lb->device_bytes = wl->slots + 1;
  hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&lb->d_labels), lb->device_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(lb->d_labels, (int)fill, lb->device_bytes, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    ibu_labels_destroy(lb);
    return hip_fail(e, "ibu_labels_create");
  }
  *out = lb;
  return IBU_OK;
}
extern "C" int32_t ibu_labels_info(const ibu_labels_t* lb, size_t* device_bytes) {
  if (!lb) return err_arg("lb is NULL");
  if (device_bytes) *device_bytes = lb->device_bytes;
  return IBU_OK;
}
extern "C" void ibu_labels_destroy(ibu_labels_t* lb) {
  if (!lb) return;
  if (lb->d_labels) {
    (void)hipSetDevice(lb->ctx->device);
    (void)hipFree(lb->d_labels);   // (waits for launches that still write or read the labels)
  }
  delete lb;
}
extern "C" int32_t ibu_labels_set(ibu_ctx_t* ctx, ibu_labels_t* lb, const uint64_t* d_codes, const uint8_t* d_labels, size_t k,
                                  size_t* n_skipped, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_labels(ctx, lb)) != 0) return rc;
  if (k > 0) {
    if ((rc = check_u64_ptr(d_codes, "d_codes")) != 0) return rc;
    if (!d_labels) return err_arg("d_labels is NULL");
    if ((rc = check_below_2_40(k, "labels_set", "codes")) != 0) return rc;
  }
  if (n_skipped) *n_skipped = 0;
  if (k == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  const auto set = [&](uint64_t* skipped) { return launch_labels_set(ctx->cfg, table_of(lb->wl), lb->d_labels, d_codes, d_labels, k, skipped, st); };
  if (!n_skipped) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(set(nullptr));
    return IBU_OK;
  }
  if ((rc = grid_totals<1>(ctx, st, set)) != 0) return rc;
  *n_skipped = ctx->h_pinned[0];
  return IBU_OK;
}
extern "C" int32_t ibu_labels_get(ibu_ctx_t* ctx, const ibu_labels_t* lb, const uint64_t* d_codes, size_t k, uint32_t missing,
                                  uint8_t* d_labels_out, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_labels(ctx, lb)) != 0) return rc;
  if ((rc = check_byte(missing, "missing")) != 0) return rc;
  if (k == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_codes, "d_codes")) != 0) return rc;
  if (!d_labels_out) return err_arg("d_labels_out is NULL");
  if ((rc = check_below_2_40(k, "labels_get", "codes")) != 0) return rc;
  IBU_HIP(launch_labels_get(ctx->cfg, table_of(lb->wl), lb->d_labels, d_codes, k, missing, d_labels_out, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_label_records(ibu_ctx_t* ctx, const ibu_labels_t* lb, const void* d_records, size_t n, uint32_t flags, uint32_t match,
                                     uint32_t missing_class, uint8_t* d_class, uint64_t* hist, void* stream) {
  if (!ctx) return no_ctx_error("labelling");   // there is no host form to fall back to
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_labels(ctx, lb)) != 0) return rc;
  if (flags & ~(uint32_t)IBU_LABEL_MATCH) return err_arg("unknown flag bit (label_records knows IBU_LABEL_MATCH)");
  if ((rc = check_byte(match, "match")) != 0) return rc;
  if ((rc = check_byte(missing_class, "missing_class")) != 0) return rc;
  if (n > 0) {
    if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
    if ((rc = check_below_2_40(n, "label_records", "records")) != 0) return rc;
  }
  if (hist) memset(hist, 0, 257 * sizeof(uint64_t));
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  const auto label = [&](uint64_t* acc) {
    return launch_label_records(ctx->cfg, table_of(lb->wl), lb->d_labels, d_records, n, (flags & IBU_LABEL_MATCH) != 0, match, missing_class,
                                d_class, acc, st);
  };
  if (!hist) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(label(nullptr));
    return IBU_OK;
  }
  if (!ctx->d_label_acc) IBU_HIP(ctx_malloc(ctx, reinterpret_cast<void**>(&ctx->d_label_acc), kLabelAccBytes));
  IBU_HIP(hipMemsetAsync(ctx->d_label_acc, 0, kLabelAccBytes, st));
  IBU_HIP(label(ctx->d_label_acc));
  IBU_HIP(launch_label_fold(ctx->d_label_acc, st));
  IBU_HIP(hipMemcpyAsync(hist, ctx->d_label_acc, 257 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  return IBU_OK;
}
extern "C" int32_t ibu_select_records(ibu_ctx_t* ctx, const void* d_records, const uint8_t* d_class, size_t n, uint32_t keep_mask,
                                      void* d_out, size_t cap, size_t* n_out, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_out) return err_arg("n_out is NULL");
  *n_out = 0;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if (!d_class) return err_arg("d_class is NULL");
  if ((rc = check_below_2_40(n, "select_records", "records")) != 0) return rc;
  const bool size_query = !d_out && cap == 0;
  if (!size_query) {
    if ((rc = check_u64_ptr(d_out, "d_out")) != 0) return rc;
    const size_t cap_in = cap < n ? cap : n;   // no more than n records are ever written
    // (cap 0 writes nothing, but a d_out that points into the records has always been refused: such a call stays refused)
    const bool empty_inside = cap_in == 0 && d_out != d_records && ranges_overlap(d_out, 1, d_records, 24 * n);
    if (ranges_overlap(d_out, 24 * cap_in, d_records, 24 * n) || empty_inside) return err_arg("d_out overlaps d_records");
  }
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_sort_scratch(ctx, select_scratch_bytes(n));
  if (rc) return rc;
  IBU_HIP(launch_select_count(ctx->cfg, d_class, n, keep_mask & 0xFFu, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back<1>(ctx, ctx->d_sort_scratch, st));
  const uint64_t kept = ctx->h_pinned[0];
  *n_out = kept;
  if (size_query) return IBU_OK;
  if (kept > cap) return err_capacity(kept, cap, "records kept", "n_out");
  IBU_HIP(launch_select_scatter(ctx->cfg, d_records, d_class, n, keep_mask & 0xFFu, ctx->d_sort_scratch, d_out, st));
  return IBU_OK;
}

// The checks ibu_partition_records makes on its map: host arithmetic, before anything else is looked at.  part_of == NULL: the
// identity below n_parts, IBU_PART_NONE above.
static int32_t partition_map(const uint8_t* part_of, uint32_t n_parts, PartitionMap* map) {
  if (n_parts < 1 || n_parts > kPartitionMaxParts)
    return set_error(IBU_ERR_INVALID_ARG, n_parts, 0, 0, "Invalid argument: n_parts must be in 1 .. 255");
  uint8_t m[256];
  for (uint32_t c = 0; c < 256; ++c) {
    const uint32_t p = part_of ? part_of[c] : (c < n_parts ? c : IBU_PART_NONE);
    if (p >= n_parts && p != IBU_PART_NONE)
      return set_error(IBU_ERR_INVALID_ARG, c, p, 0, "Invalid argument: part_of[%u] = %u is neither below n_parts nor IBU_PART_NONE", c, p);
    m[c] = (uint8_t)p;
  }
  memcpy(map->w, m, sizeof m);
  return IBU_OK;
}
extern "C" int32_t ibu_partition_records(ibu_ctx_t* ctx, const void* d_records, const uint8_t* d_class, size_t n, const uint8_t part_of[256],
                                         uint32_t n_parts, void* d_out, size_t cap, uint64_t* offsets, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  PartitionMap map;
  if ((rc = partition_map(part_of, n_parts, &map)) != 0) return rc;
  if (!offsets) return err_arg("offsets is NULL");
  memset(offsets, 0, (n_parts + 1) * sizeof(uint64_t));
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if (!d_class) return err_arg("d_class is NULL");
  if ((rc = check_below_2_40(n, "partition_records", "records")) != 0) return rc;
  const bool size_query = !d_out && cap == 0;
  if (!size_query) {
    if ((rc = check_u64_ptr(d_out, "d_out")) != 0) return rc;
    const size_t cap_in = cap < n ? cap : n;   // no more than n records are ever written
    const bool empty_inside = cap_in == 0 && d_out != d_records && ranges_overlap(d_out, 1, d_records, 24 * n);   // (as ibu_select_records)
    if (ranges_overlap(d_out, 24 * cap_in, d_records, 24 * n) || empty_inside) return err_arg("d_out overlaps d_records");
  }
  const PartitionPlan pl = partition_plan(n, n_parts);
  if (!pl.ok)
    return set_error(IBU_ERR_INVALID_ARG, pl.entries, kPartitionMaxEntries, 0,
                     "Invalid argument: partition_records: %llu parts x units is more than one scan takes (%llu): split the records",
                     (unsigned long long)pl.entries, (unsigned long long)kPartitionMaxEntries);
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_sort_scratch(ctx, pl.scratch_bytes);
  if (rc) return rc;
  IBU_HIP(launch_partition_count(ctx->cfg, d_class, n, n_parts, map, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back_words(ctx, static_cast<const uint64_t*>(ctx->d_sort_scratch) + 1 + pl.entries, n_parts + 1, st));
  memcpy(offsets, ctx->h_pinned, (n_parts + 1) * sizeof(uint64_t));
  const uint64_t kept = offsets[n_parts];
  if (size_query) return IBU_OK;
  if (kept > cap) return err_capacity(kept, cap, "records kept", "offsets[n_parts]");
  IBU_HIP(launch_partition_scatter(ctx->cfg, d_records, d_class, n, n_parts, map, ctx->d_sort_scratch, d_out, st));
  return IBU_OK;
}
