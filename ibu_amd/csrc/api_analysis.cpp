// api_analysis.cpp — the entry points of the C ABI (include/ibu_hip.h) that analyse sorted records: the run-length aggregations
// (barcode and pair counts, the count matrix), molecules, cells, the per-barcode and per-feature metrics and filters, subsampling and the
// saturation curve.  Most are a count pass, its totals read back, and an emit pass on a scratch sized by them.
#include <stddef.h>

#include "ctx.hpp"

using namespace ibu;

// the emit scratch of the run-length aggregations (16 bytes per entry): grows only
static int32_t ensure_runs_scratch(ibu_ctx* ctx, size_t need) {
  if (need <= ctx->runs_scratch_bytes) return IBU_OK;
  if (ctx->d_runs_scratch) IBU_HIP(hipFree(ctx->d_runs_scratch));
  ctx->d_runs_scratch = nullptr;
  ctx->runs_scratch_bytes = 0;
  IBU_HIP(ctx_malloc(ctx, &ctx->d_runs_scratch, need));
  ctx->runs_scratch_bytes = need;
  return IBU_OK;
}
// The first half of every run-length aggregation: a count scratch of `need` bytes, the count pass, and its two totals (runs, ranked
// heads) read back into ctx->h_pinned[0..1].  Synchronises the stream.
static int32_t runs_count_totals(ibu_ctx* ctx, const void* d_sorted_records, size_t n, size_t need, RunsCount what, hipStream_t st) {
  int32_t rc = ensure_sort_scratch(ctx, need);
  if (rc) return rc;
  IBU_HIP(launch_runs_count(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->sort_scratch_bytes, what, st));
  IBU_HIP(read_back<2>(ctx, ctx->d_sort_scratch, st));
  return IBU_OK;
}
// BarcodeAnalyzer (parallel.rs:72-98) on sorted device records.
extern "C" int32_t ibu_barcode_counts(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t* d_barcodes,
                                      uint64_t* d_counts, uint64_t* d_unique_umis, size_t cap, size_t* n_barcodes,
                                      size_t* n_barcode_umi_pairs, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_barcodes) return err_arg("n_barcodes is NULL");
  *n_barcodes = 0;
  if (n_barcode_umi_pairs) *n_barcode_umi_pairs = 0;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_sorted_records, "d_sorted_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "barcode_counts", "records")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  const bool size_query = !d_barcodes && !d_counts && cap == 0;
  // (with outputs to fill, the count pass keeps every segment's first few run heads: the emit pass then reads the records again only
  // where runs are short — k_aggregate.hip)
  rc = runs_count_totals(ctx, d_sorted_records, n, runs_scratch_bytes(n), size_query ? RunsCount::Barcode : RunsCount::BarcodeStash, st);
  if (rc) return rc;
  const uint64_t runs = ctx->h_pinned[0], pairs = ctx->h_pinned[1];
  *n_barcodes = runs;
  if (n_barcode_umi_pairs) *n_barcode_umi_pairs = pairs;
  if (size_query) return IBU_OK;
  if (!d_barcodes || !d_counts) return err_arg("d_barcodes / d_counts are NULL");
  if (runs > cap) return err_arg("output capacity is smaller than the number of distinct barcodes (see *n_barcodes)");
  rc = ensure_runs_scratch(ctx, runs_emit_scratch_bytes(runs));
  if (rc) return rc;
  IBU_HIP(launch_runs_emit(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, runs, pairs, d_barcodes, nullptr,
                           d_counts, d_unique_umis, st));
  return IBU_OK;
}
// ---- count matrix: distinct UMIs and reads per (barcode, index) pair (k_records.hip: the field exchange; k_aggregate.hip: the
// pair-level run walk).  The semantics are this library's: include/ibu_hip.h.
extern "C" int32_t ibu_records_swap_umi_index(ibu_ctx_t* ctx, const void* d_src, void* d_dst, size_t n, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptrs({d_src, d_dst}, "d_src / d_dst")) != 0) return rc;
  if ((rc = check_below_2_40(n, "records_swap_umi_index", "records")) != 0) return rc;
  if (d_dst != d_src && ranges_overlap(d_dst, 24 * n, d_src, 24 * n))
    return err_arg("d_dst overlaps d_src (only d_dst == d_src, in place, is allowed)");
  IBU_HIP(launch_swap_fields(ctx->cfg, d_src, d_dst, n, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_pair_counts(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t* d_first, uint64_t* d_second,
                                   uint64_t* d_records_per_pair, uint64_t* d_distinct_third, size_t cap, size_t* n_pairs,
                                   size_t* n_triples, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_pairs) return err_arg("n_pairs is NULL");
  *n_pairs = 0;
  if (n_triples) *n_triples = 0;
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_sorted_records, "d_sorted_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "pair_counts", "records")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  rc = runs_count_totals(ctx, d_sorted_records, n, runs_scratch_bytes(n), RunsCount::Pair, st);
  if (rc) return rc;
  const bool size_query = !d_first && !d_second && !d_records_per_pair && cap == 0;
  const uint64_t pairs = ctx->h_pinned[0], triples = ctx->h_pinned[1];
  *n_pairs = pairs;
  if (n_triples) *n_triples = triples;
  if (size_query) return IBU_OK;
  if (!d_first || !d_second || !d_records_per_pair) return err_arg("d_first / d_second / d_records_per_pair are NULL");
  if (!aligned8(d_first) || !aligned8(d_second) || !aligned8(d_records_per_pair) || !aligned8(d_distinct_third))
    return err_arg("the output arrays must be 8-byte aligned");
  if (pairs > cap) return err_capacity(pairs, cap, "entries", "n_pairs");
  rc = ensure_runs_scratch(ctx, runs_emit_scratch_bytes(pairs));
  if (rc) return rc;
  IBU_HIP(launch_runs_emit(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, pairs, triples, d_first, d_second,
                           d_records_per_pair, d_distinct_third, st));
  return IBU_OK;
}
// One index per (w0, w1) molecule: the candidate with strictly the most records (k_molecules.hip; the rule: include/ibu_hip.h).
extern "C" int32_t ibu_classify_molecules(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint32_t flags, uint8_t* d_class,
                                          ibu_molecule_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (flags & ~(uint32_t)IBU_MOLECULES_TIE_FIRST) return err_arg("unknown bit in flags");
  if (counts) *counts = ibu_molecule_counts_t{0, 0, 0, 0, 0, 0, 0, 0};
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_sorted_records, "d_sorted_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "classify_molecules", "records")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  rc = runs_count_totals(ctx, d_sorted_records, n, molecules_scratch_bytes(n), RunsCount::Pair, st);
  if (rc) return rc;
  const uint64_t molecules = ctx->h_pinned[0], candidates = ctx->h_pinned[1];
  rc = ensure_runs_scratch(ctx, molecules_run_scratch_bytes(candidates));
  if (rc) return rc;
  IBU_HIP(launch_molecules_classify(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, candidates,
                                    (flags & IBU_MOLECULES_TIE_FIRST) != 0, d_class, st));
  if (!counts) return IBU_OK;
  IBU_HIP(read_back<5>(ctx, ctx->d_runs_scratch, st));
  counts->molecules = molecules;
  counts->candidates = candidates;
  counts->resolved = ctx->h_pinned[0];
  counts->tied = ctx->h_pinned[1];
  counts->reads_kept = ctx->h_pinned[2];
  counts->reads_minor = ctx->h_pinned[3];
  counts->reads_tied = ctx->h_pinned[4];
  return IBU_OK;
}
// Which barcodes are cells: one threshold on the per-barcode UMI (or read) count (k_cells.hip; the rule: include/ibu_hip.h).
extern "C" int32_t ibu_call_cells(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint32_t mode, uint64_t param, uint32_t flags,
                                  uint8_t* d_class, ibu_cell_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (mode > IBU_CELLS_ORDMAG) return err_arg("unknown mode");
  if (flags & ~(uint32_t)IBU_CELLS_BY_READS) return err_arg("unknown bit in flags");
  if (mode != IBU_CELLS_MIN && param == 0) return err_arg("param must be at least 1 in the TOP and ORDMAG modes");
  if (n && (rc = check_u64_ptr(d_sorted_records, "d_sorted_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "call_cells", "records")) != 0) return rc;
  if (counts) {   // (behind the last argument check: a refused call leaves the totals alone)
    *counts = ibu_cell_counts_t{0, 0, 0, 0, 0, 0, 0, 0};
    if (mode == IBU_CELLS_MIN) counts->threshold = param;
  }
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  rc = runs_count_totals(ctx, d_sorted_records, n, cells_scratch_bytes(n), RunsCount::Barcode, st);
  if (rc) return rc;
  const uint64_t barcodes = ctx->h_pinned[0], pairs = ctx->h_pinned[1];
  rc = ensure_runs_scratch(ctx, cells_run_scratch_bytes(barcodes));
  if (rc) return rc;
  IBU_HIP(launch_cells_call(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, barcodes, pairs, mode, param,
                            (flags & IBU_CELLS_BY_READS) != 0, d_class, st));
  if (!counts) return IBU_OK;
  IBU_HIP(read_back<7>(ctx, ctx->d_runs_scratch, st));
  counts->barcodes = barcodes;
  counts->cells = ctx->h_pinned[0];
  counts->reads_cells = ctx->h_pinned[1];
  counts->reads_background = ctx->h_pinned[2];
  counts->umis_cells = ctx->h_pinned[3];
  counts->umis_background = ctx->h_pinned[4];
  counts->threshold = ctx->h_pinned[5];
  counts->baseline = ctx->h_pinned[6];
  return IBU_OK;
}
// ---- per-barcode QC metrics and the barcode filter (k_metrics.hip).  The semantics are this library's: include/ibu_hip.h.
static_assert(sizeof(ibu_barcode_limits_t) == sizeof(MetricsLimits) && offsetof(ibu_barcode_limits_t, set_of) == offsetof(MetricsLimits, set_of) &&
                  offsetof(ibu_barcode_limits_t, set_num) == offsetof(MetricsLimits, set_num) && sizeof(ibu_barcode_filter_counts_t) == 96,
              "ibu_hip.h and kernels.h disagree");
static int32_t check_feature_set(const uint64_t* d_set, uint64_t set_bits, uint32_t set_word) {
  if (!metrics_set_ok(d_set, set_bits, set_word))
    return err_arg("the feature set: set_word must be 1 or 2, set_bits at most 2^32, d_set 8-byte aligned and non-NULL unless set_bits is 0");
  return IBU_OK;
}
// The first half of both: the count pass and its five totals read back into ctx->h_pinned[0..4].  Synchronises the stream.
static int32_t metrics_count_totals(ibu_ctx* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits, uint32_t set_word,
                                    hipStream_t st) {
  int32_t rc = ensure_sort_scratch(ctx, metrics_scratch_bytes(n));
  if (rc) return rc;
  IBU_HIP(launch_metrics_count(ctx->cfg, d_records, n, d_set, set_bits, set_word, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back<5>(ctx, ctx->d_sort_scratch, st));
  return IBU_OK;
}
extern "C" int32_t ibu_barcode_metrics(ibu_ctx_t* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits,
                                       uint32_t set_word, uint64_t* d_barcodes, uint64_t* d_reads, uint64_t* d_pairs, uint64_t* d_triples,
                                       uint64_t* d_set_reads, uint64_t* d_set_triples, size_t cap, size_t* n_barcodes, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_barcodes) return err_arg("n_barcodes is NULL");
  if ((rc = check_feature_set(d_set, set_bits, set_word)) != 0) return rc;
  if ((rc = check_below_2_40(n, "barcode_metrics", "records")) != 0) return rc;
  if (n && (rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if (n && (!aligned8(d_barcodes) || !aligned8(d_reads) || !aligned8(d_pairs) || !aligned8(d_triples) || !aligned8(d_set_reads) ||
            !aligned8(d_set_triples)))
    return err_arg("the output arrays must be 8-byte aligned");
  *n_barcodes = 0;
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  rc = metrics_count_totals(ctx, d_records, n, d_set, set_bits, set_word, st);
  if (rc) return rc;
  const uint64_t barcodes = ctx->h_pinned[0];
  *n_barcodes = barcodes;
  const bool any_column = d_barcodes || d_reads || d_pairs || d_triples || d_set_reads || d_set_triples;
  if (!any_column) return IBU_OK;   // the size query (cap == 0), or a cap and nothing to write
  if (barcodes > cap) return err_capacity(barcodes, cap, "barcodes", "n_barcodes");
  rc = ensure_runs_scratch(ctx, metrics_run_scratch_bytes(barcodes));
  if (rc) return rc;
  IBU_HIP(launch_metrics_table(ctx->cfg, d_records, n, d_set, set_bits, set_word, ctx->d_sort_scratch, ctx->d_runs_scratch, barcodes, d_barcodes,
                               d_reads, d_pairs, d_triples, d_set_reads, d_set_triples, st));
  return IBU_OK;
}
extern "C" int32_t ibu_filter_barcodes(ibu_ctx_t* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits,
                                       uint32_t set_word, const ibu_barcode_limits_t* limits, uint8_t* d_class,
                                       ibu_barcode_filter_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_feature_set(d_set, set_bits, set_word)) != 0) return rc;
  if (!limits) return err_arg("limits is NULL");
  const MetricsLimits lim{limits->min_reads, limits->max_reads, limits->min_pairs, limits->max_pairs, limits->min_triples, limits->max_triples,
                          limits->set_num, limits->set_den, limits->set_of, 0};
  if (!metrics_limits_ok(lim)) return err_arg("limits: set_of must be 0 (reads) or 1 (triples), and set_num <= set_den < 2^24");
  if (n && (rc = check_u64_ptr(d_records, "d_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "filter_barcodes", "records")) != 0) return rc;
  if (counts) *counts = ibu_barcode_filter_counts_t{};   // (behind the last argument check: a refused call leaves the totals alone)
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  rc = metrics_count_totals(ctx, d_records, n, d_set, set_bits, set_word, st);
  if (rc) return rc;
  const uint64_t barcodes = ctx->h_pinned[0];
  rc = ensure_runs_scratch(ctx, metrics_run_scratch_bytes(barcodes));
  if (rc) return rc;
  IBU_HIP(launch_metrics_filter(ctx->cfg, d_records, n, d_set, set_bits, set_word, ctx->d_sort_scratch, ctx->d_runs_scratch, barcodes, lim, d_class, st));
  if (!counts) return IBU_OK;
  IBU_HIP(read_back<10>(ctx, ctx->d_runs_scratch, st));
  counts->barcodes = barcodes;
  for (int c = 0; c < 4; ++c) {
    counts->barcodes_by_class[c] = ctx->h_pinned[c];
    counts->reads_by_class[c] = ctx->h_pinned[4 + c];
  }
  counts->triples_passed = ctx->h_pinned[8];
  counts->set_triples_passed = ctx->h_pinned[9];
  return IBU_OK;
}
// ---- per-feature metrics and the feature filter (k_features.hip).  The semantics are this library's: include/ibu_hip.h.
static_assert(sizeof(ibu_feature_limits_t) == sizeof(FeatureLimits) && offsetof(ibu_feature_limits_t, min_cells) == offsetof(FeatureLimits, min_cells) &&
                  sizeof(ibu_feature_filter_counts_t) == 64,
              "ibu_hip.h and kernels.h disagree");
// what both calls check first: the feature word, the table size, the columns' alignment, the records
static int32_t check_feature_call(const char* fn, const void* d_records, size_t n, uint32_t feature_word, uint64_t n_features,
                                  const uint64_t* d_reads, const uint64_t* d_umis, const uint64_t* d_cells) {
  if (!feature_args_ok(feature_word, n_features)) return err_arg("feature_word must be 1 or 2 and n_features in 1 .. 2^32");
  if (!aligned8(d_reads) || !aligned8(d_umis) || !aligned8(d_cells)) return err_arg("the columns must be 8-byte aligned");
  int32_t rc = check_below_2_40(n, fn, "records");
  if (rc) return rc;
  return n ? check_u64_ptr(d_records, "d_records") : IBU_OK;
}
extern "C" int32_t ibu_feature_metrics(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t feature_word, uint64_t n_features,
                                       uint32_t flags, uint64_t* d_reads, uint64_t* d_umis, uint64_t* d_cells, uint64_t totals[4], void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_feature_call("feature_metrics", d_records, n, feature_word, n_features, d_reads, d_umis, d_cells)) != 0) return rc;
  if (flags & ~(uint32_t)IBU_FEATURE_ACCUMULATE) return err_arg("unknown bit in flags");
  if (feature_word == 2 && d_cells) return err_arg("d_cells needs feature_word 1: cells are not available on records sorted by (barcode, umi, index)");
  hipStream_t st = pick_stream(ctx, stream);
  if (!(flags & IBU_FEATURE_ACCUMULATE))
    for (uint64_t* col : {d_reads, d_umis, d_cells})
      if (col) IBU_HIP(hipMemsetAsync(col, 0, sizeof(uint64_t) * n_features, st));
  const auto count = [&](uint64_t* acc) { return launch_feature_count(ctx->cfg, d_records, n, feature_word, n_features, d_reads, d_umis, d_cells, acc, st); };
  if (!totals) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(count(nullptr));
    return IBU_OK;
  }
  if ((rc = grid_totals<4>(ctx, st, count)) != 0) return rc;
  for (int k = 0; k < 4; ++k) totals[k] = ctx->h_pinned[k];
  return IBU_OK;
}
extern "C" int32_t ibu_filter_features(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t feature_word, uint64_t n_features,
                                       const uint64_t* d_reads, const uint64_t* d_umis, const uint64_t* d_cells,
                                       const ibu_feature_limits_t* limits, uint8_t* d_class, uint8_t* d_verdict,
                                       ibu_feature_filter_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_feature_call("filter_features", d_records, n, feature_word, n_features, d_reads, d_umis, d_cells)) != 0) return rc;
  if (!limits) return err_arg("limits is NULL");
  if ((!d_reads && (limits->min_reads || limits->max_reads)) || (!d_umis && (limits->min_umis || limits->max_umis)) ||
      (!d_cells && (limits->min_cells || limits->max_cells)))
    return err_arg("a column with a non-zero limit is NULL");
  const FeatureLimits lim{limits->min_reads, limits->max_reads, limits->min_umis, limits->max_umis, limits->min_cells, limits->max_cells};
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_runs_scratch(ctx, feature_run_scratch_bytes(d_verdict ? 0 : n_features));
  if (rc) return rc;
  uint64_t* acc = static_cast<uint64_t*>(ctx->d_runs_scratch);
  uint8_t* verdict = d_verdict ? d_verdict : static_cast<uint8_t*>(ctx->d_runs_scratch) + kFeatureAccBytes;
  IBU_HIP(launch_feature_filter(ctx->cfg, d_records, n, feature_word, n_features, d_reads, d_umis, d_cells, lim, verdict, d_class, counts != nullptr,
                                acc, st));
  if (!counts) return IBU_OK;
  IBU_HIP(read_back<8>(ctx, acc, st));
  *counts = ibu_feature_filter_counts_t{};
  for (int v = 0; v < 3; ++v) counts->features_by_class[v] = ctx->h_pinned[v];
  for (int c = 0; c < 4; ++c) counts->reads_by_class[c] = ctx->h_pinned[4 + c];
  return IBU_OK;
}
// ---- read subsampling and the saturation curve (k_saturation.hip).  The semantics are this library's: include/ibu_hip.h.
extern "C" int32_t ibu_subsample_class(ibu_ctx_t* ctx, size_t n, uint64_t first_row, uint64_t seed, uint64_t threshold, uint8_t* d_class,
                                       size_t* n_kept, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!d_class && !n_kept) return err_arg("d_class and n_kept are both NULL: nothing to do");
  if ((rc = check_below_2_40(n, "subsample_class", "rows")) != 0) return rc;
  if (n_kept) *n_kept = 0;
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  const uint64_t base = sample_base(seed, first_row);
  if (!n_kept) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(launch_subsample(ctx->cfg, n, base, threshold, d_class, nullptr, st));
    return IBU_OK;
  }
  rc = grid_totals<1>(ctx, st, [&](uint64_t* acc) { return launch_subsample(ctx->cfg, n, base, threshold, d_class, acc, st); });
  if (rc) return rc;
  *n_kept = ctx->h_pinned[0];
  return IBU_OK;
}
extern "C" int32_t ibu_saturation_curve(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t first_row, uint64_t seed,
                                        const uint64_t* thresholds, uint32_t k, ibu_saturation_point_t* points, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (k == 0 || k > IBU_SATURATION_MAX_POINTS) return err_arg("k must be 1..32");
  if (!thresholds || !points) return err_arg("thresholds / points are NULL");
  for (uint32_t j = 1; j < k; ++j)
    if (thresholds[j] < thresholds[j - 1]) return err_arg("the thresholds must be non-decreasing");
  if (n && (rc = check_u64_ptr(d_sorted_records, "d_sorted_records")) != 0) return rc;
  if ((rc = check_below_2_40(n, "saturation_curve", "records")) != 0) return rc;
  if (n == 0) {
    for (uint32_t j = 0; j < k; ++j) points[j] = ibu_saturation_point_t{thresholds[j], 0, 0, 0};
    return IBU_OK;
  }
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_sort_scratch(ctx, saturation_scratch_bytes(n));
  if (rc) return rc;
  IBU_HIP(launch_saturation(ctx->cfg, d_sorted_records, n, sample_base(seed, first_row), thresholds, k, ctx->d_sort_scratch,
                            ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back<3 * kSaturationMaxPoints>(ctx, static_cast<const uint8_t*>(ctx->d_sort_scratch) + saturation_points_offset(), st));
  for (uint32_t j = 0; j < k; ++j)
    points[j] = ibu_saturation_point_t{thresholds[j], ctx->h_pinned[j], ctx->h_pinned[kSaturationMaxPoints + j],
                                       ctx->h_pinned[2 * kSaturationMaxPoints + j]};
  return IBU_OK;
}
// TEST HOOK, not part of the ABI (not declared in include/ibu_hip.h, no binding): the selection ibu_call_cells runs, on a caller's
// array — *value = the rank-th largest (1 <= rank <= n) of n device values below 2^40.  Records cannot reach the digit passes above
// bit 31 at any size a test can afford; tests/test_gpu_cells.py reaches them through this.  Synchronises.
extern "C" int32_t ibu_test_rank_select(ibu_ctx_t* ctx, const uint64_t* d_values, size_t n, uint64_t rank, uint64_t* value, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!value) return err_arg("value is NULL");
  if (n == 0 || rank == 0 || rank > n) return err_arg("rank must be in 1..n");
  if ((rc = check_u64_ptr(d_values, "d_values")) != 0) return rc;
  if ((rc = check_below_2_40(n, "rank_select", "values")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_runs_scratch(ctx, rank_select_work_bytes());
  if (rc) return rc;
  IBU_HIP(launch_rank_select(ctx->cfg, d_values, n, rank, ctx->d_runs_scratch, st));
  IBU_HIP(read_back<1>(ctx, ctx->d_runs_scratch, st));
  *value = ctx->h_pinned[0];
  return IBU_OK;
}
extern "C" int32_t ibu_count_matrix(ibu_ctx_t* ctx, void* d_records, void* d_tmp, size_t n, uint32_t flags, uint64_t* d_barcodes,
                                    uint64_t* d_indices, uint64_t* d_reads, uint64_t* d_umis, size_t cap, size_t* n_entries,
                                    size_t* n_molecules, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_entries) return err_arg("n_entries is NULL");
  *n_entries = 0;
  if (n_molecules) *n_molecules = 0;
  if (flags & ~(uint32_t)IBU_COUNT_LEAVE_SWAPPED) return err_arg("unknown bit in flags");
  if (n == 0) return IBU_OK;
  if ((rc = check_u64_ptrs({d_records, d_tmp}, "d_records / d_tmp")) != 0) return rc;
  if (!d_barcodes || !d_indices || !d_reads) return err_arg("d_barcodes / d_indices / d_reads are NULL");
  if (!aligned8(d_barcodes) || !aligned8(d_indices) || !aligned8(d_reads) || !aligned8(d_umis))
    return err_arg("the output arrays must be 8-byte aligned");
  if ((rc = check_below_2_40(n, "count_matrix", "records")) != 0) return rc;
  if ((rc = ibu_records_swap_umi_index(ctx, d_records, d_records, n, stream)) != 0) return rc;
  if ((rc = ibu_sort_records(ctx, d_records, d_tmp, n, stream)) != 0) return rc;
  // a capacity that is too small is reported once the records are back in the state the flags promise
  const int32_t rc_counts = ibu_pair_counts(ctx, d_records, n, d_barcodes, d_indices, d_reads, d_umis, cap, n_entries, n_molecules, stream);
  if (!(flags & IBU_COUNT_LEAVE_SWAPPED) && (rc_counts == IBU_OK || rc_counts == IBU_ERR_INVALID_ARG))
    if ((rc = ibu_records_swap_umi_index(ctx, d_records, d_records, n, stream)) != 0) return rc;
  return rc_counts;
}
// ---- the matrix export (k_matrix.hip): the row structure of a column of the entry table, and three columns as decimal text.  The
// semantics are this library's: include/ibu_hip.h.  Both are a count pass and its scan on the context's sort scratch, the totals read
// back, and a scatter pass.
extern "C" int32_t ibu_matrix_rows(ibu_ctx_t* ctx, const uint64_t* d_first, size_t n_entries, uint64_t* d_row_of_entry, uint64_t* d_row_keys,
                                   uint64_t* d_row_ptr, size_t cap, size_t* n_rows, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_rows) return err_arg("n_rows is NULL");
  *n_rows = 0;
  if (n_entries == 0) return IBU_OK;
  if ((rc = check_u64_ptr(d_first, "d_first")) != 0) return rc;
  if ((rc = check_below_2_40(n_entries, "matrix_rows", "entries")) != 0) return rc;
  if (!aligned8(d_row_of_entry) || !aligned8(d_row_keys) || !aligned8(d_row_ptr)) return err_arg("the output arrays must be 8-byte aligned");
  hipStream_t st = pick_stream(ctx, stream);
  if ((rc = ensure_sort_scratch(ctx, matrix_scratch_bytes(n_entries))) != 0) return rc;
  IBU_HIP(launch_matrix_rows_count(ctx->cfg, d_first, n_entries, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back<1>(ctx, static_cast<const uint64_t*>(ctx->d_sort_scratch) + kMatrixTotalWord, st));
  const uint64_t rows = ctx->h_pinned[0];
  *n_rows = rows;
  if (!d_row_of_entry && !d_row_keys && !d_row_ptr) return IBU_OK;   // the size query (cap == 0), or nothing asked for
  if (rows > cap) return err_capacity(rows, cap, "rows", "n_rows");
  IBU_HIP(launch_matrix_rows_scatter(ctx->cfg, d_first, n_entries, ctx->d_sort_scratch, d_row_of_entry, d_row_keys, d_row_ptr, st));
  return IBU_OK;
}
extern "C" int32_t ibu_matrix_market_body(ibu_ctx_t* ctx, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, size_t n_entries,
                                          uint64_t add_a, uint64_t add_b, char* d_text, size_t cap_bytes, size_t* n_bytes, uint64_t maxima[3],
                                          void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_bytes) return err_arg("n_bytes is NULL");
  *n_bytes = 0;
  if (maxima) maxima[0] = maxima[1] = maxima[2] = 0;
  if (n_entries == 0) return IBU_OK;
  if ((rc = check_u64_ptrs({d_a, d_b, d_c}, "d_a / d_b / d_c")) != 0) return rc;
  if ((rc = check_below_2_40(n_entries, "matrix_market_body", "entries")) != 0) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  if ((rc = ensure_sort_scratch(ctx, matrix_scratch_bytes(n_entries))) != 0) return rc;
  IBU_HIP(launch_matrix_text_count(ctx->cfg, d_a, d_b, d_c, n_entries, add_a, add_b, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back<kMatrixTotalWord + 1>(ctx, ctx->d_sort_scratch, st));
  const uint64_t bytes = ctx->h_pinned[kMatrixTotalWord];
  *n_bytes = bytes;
  if (maxima)
    for (int k = 0; k < 3; ++k) maxima[k] = ctx->h_pinned[k];
  if (!d_text && cap_bytes == 0) return IBU_OK;   // the size query
  if (!d_text) return err_arg("d_text is NULL");
  if (bytes > cap_bytes) return err_capacity(bytes, cap_bytes, "bytes of text", "n_bytes");
  for (const uint64_t* col : {d_a, d_b, d_c})
    if (ranges_overlap(d_text, bytes, col, 8 * n_entries)) return err_arg("d_text overlaps an input column");
  IBU_HIP(launch_matrix_text_write(ctx->cfg, d_a, d_b, d_c, n_entries, add_a, add_b, ctx->d_sort_scratch, d_text, st));
  return IBU_OK;
}
// ---- the per-row top-2 and the class of a row (k_matrix.hip).  The semantics are this library's: include/ibu_hip.h.  The count pass
// and scan of ibu_matrix_rows give the row ordinals, the row total comes back, then a reduce pass and a finishing pass.
extern "C" int32_t ibu_matrix_row_top(ibu_ctx_t* ctx, const uint64_t* d_first, const uint64_t* d_second, const uint64_t* d_values,
                                      size_t n_entries, const uint64_t* d_set, uint64_t set_bits, uint64_t* d_top_key, uint64_t* d_top_value,
                                      uint64_t* d_next_value, uint64_t* d_row_sum, uint64_t* d_row_entries, size_t cap, size_t* n_rows,
                                      void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_rows) return err_arg("n_rows is NULL");
  if (!d_set && set_bits) return err_arg("d_set is NULL and set_bits is not 0");
  if (set_bits > (1ull << 32) || !aligned8(d_set)) return err_arg("the feature set: set_bits at most 2^32, d_set 8-byte aligned");
  *n_rows = 0;
  if (n_entries == 0) return IBU_OK;
  if ((rc = check_u64_ptrs({d_first, d_second, d_values}, "d_first / d_second / d_values")) != 0) return rc;
  if ((rc = check_below_2_40(n_entries, "matrix_row_top", "entries")) != 0) return rc;
  uint64_t* const outs[5] = {d_top_key, d_top_value, d_next_value, d_row_sum, d_row_entries};
  for (const uint64_t* o : outs)
    if (!aligned8(o)) return err_arg("the output arrays must be 8-byte aligned");
  hipStream_t st = pick_stream(ctx, stream);
  if ((rc = ensure_sort_scratch(ctx, row_top_scratch_bytes(n_entries))) != 0) return rc;
  IBU_HIP(launch_matrix_rows_count(ctx->cfg, d_first, n_entries, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(read_back<1>(ctx, static_cast<const uint64_t*>(ctx->d_sort_scratch) + kMatrixTotalWord, st));
  const uint64_t rows = ctx->h_pinned[0];
  *n_rows = rows;
  if (!d_top_key && !d_top_value && !d_next_value && !d_row_sum && !d_row_entries) return IBU_OK;   // the size query, whatever cap says
  if (rows > cap) return err_capacity(rows, cap, "rows", "n_rows");
  for (int a = 0; a < 5; ++a) {
    if (!outs[a]) continue;
    for (const uint64_t* col : {d_first, d_second, d_values})
      if (ranges_overlap(outs[a], 8 * rows, col, 8 * n_entries)) return err_arg("an output overlaps an input column");
    for (int b = a + 1; b < 5; ++b)
      if (outs[b] && ranges_overlap(outs[a], 8 * rows, outs[b], 8 * rows)) return err_arg("two outputs overlap");
  }
  IBU_HIP(launch_matrix_row_top(ctx->cfg, d_first, d_second, d_values, n_entries, d_set, set_bits, ctx->d_sort_scratch,
                                ctx->sort_scratch_bytes, d_top_key, d_top_value, d_next_value, d_row_sum, d_row_entries, st));
  return IBU_OK;
}
extern "C" int32_t ibu_assign_rows(ibu_ctx_t* ctx, const uint64_t* d_top_value, const uint64_t* d_next_value, const uint64_t* d_row_sum,
                                   size_t n_rows, const ibu_assign_rule_t* rule, uint8_t* d_row_class, ibu_assign_counts_t* counts,
                                   void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!rule) return err_arg("rule is NULL");
  if (rule->den == 0 || rule->num > rule->den) return err_arg("rule: den must be at least 1 and num at most den");
  if (!d_row_class && !counts) return err_arg("d_row_class and counts are both NULL: nothing to do");
  if ((rc = check_below_2_40(n_rows, "assign_rows", "rows")) != 0) return rc;
  if (n_rows && (rc = check_u64_ptrs({d_top_value, d_next_value, d_row_sum}, "d_top_value / d_next_value / d_row_sum")) != 0) return rc;
  if (counts) *counts = ibu_assign_counts_t{0, 0, 0, 0};   // (behind the last argument check: a refused call leaves the totals alone)
  if (n_rows == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  const auto assign = [&](uint64_t* acc) {
    return launch_matrix_assign(ctx->cfg, d_top_value, d_next_value, d_row_sum, n_rows, rule->min_value, rule->num, rule->den, d_row_class, acc, st);
  };
  if (!counts) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(assign(nullptr));
    return IBU_OK;
  }
  if ((rc = grid_totals<3>(ctx, st, assign)) != 0) return rc;
  counts->rows = n_rows;
  counts->assigned = ctx->h_pinned[IBU_ROW_ASSIGNED];
  counts->none = ctx->h_pinned[IBU_ROW_NONE];
  counts->mixed = ctx->h_pinned[IBU_ROW_MIXED];
  return IBU_OK;
}
