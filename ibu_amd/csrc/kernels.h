// kernels.h — launch interface between the C-ABI layer (device.cpp, api_*.cpp) and the k_*.hip kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

namespace ibu {

struct LaunchCfg {
  int cus = 256;           // hipDeviceProp_t::multiProcessorCount
  int blocks_per_cu = 7;   // persistent grid = cus * blocks_per_cu workgroups of 256 threads (7 beats 8: profiles/r01_c)
  int sort_variant = 0;    // tile shape / write-out mode of the radix passes (sort.hip kSweep; A/B knob)
  int sort_guess = 1;      // compact-key sorts compress on a SAMPLED guess of the varying bytes while the exact census runs in the same pass: 0 = never, 1 = from 2^17 records (the default), k = from k records
  int sort_compact = 1;    // compact-key passes (12-byte elements when at most 12 key bytes vary): 0 = never, k = tile shape kCompact[k-1]
  int sort_hybrid = 1;     // wide keys (more than 16 varying bytes): LSD over the top P varying bytes only, then ONE finishing pass that completes every run of equal prefix in LDS (sort.hip, ibu_k_sort_finish): 0 = never, 1 = when at least three passes are saved, 2 = whenever one is (tests)
  int sort_idx64 = 0;      // test knob: 1 = the sort indexes with 64 bits at any size (the kernels inputs of 2^32 records and more take)
  int alloc_probe_tries = 0; // placement probing inside the library, for resident arrays the library allocates (ibu_device_alloc, ibu_load_to_device's destination, the sort scratch): 0 = auto (>= 1 GiB and at least three candidates fit: up to four), 1 = plain hipMalloc, k = allocations of at least 256 MiB draw k candidates and keep the fastest (device.cpp: ibu_device_alloc_probed)
  int trace_rows = 0;      // tests: one stderr line per launch saying how many rows took the tiled / the tail kernel (kcommon.hpp: split_rows)
  uint32_t base_order = 0; // bit order of the 2-bit codec: 0 = base i at bits [2i,2i+1] (default), 1 = first base most significant
};

// Persistent grids must be exactly resident: a workgroup that has to wait for a slot runs its
// whole share alone at the end (measured: decode 5.07 -> 5.6 TB/s once fixed).  Ask the runtime
// how many 256-thread blocks of this kernel fit on a CU (registers, LDS), cap by
// cfg.blocks_per_cu, remember the answer per kernel instantiation.
template <int BLOCK, class K>
static inline int resident_blocks(const LaunchCfg& cfg, K kernel, size_t dyn_lds, std::atomic<int>* cache) {
  int cached = cache->load(std::memory_order_relaxed);  // contexts of several host threads may race here: same value either way
  if (cached <= 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, BLOCK, dyn_lds) != hipSuccess || nb <= 0)
      nb = 1024 / BLOCK;
    cache->store(nb, std::memory_order_relaxed);
    cached = nb;
  }
  int cap = cfg.blocks_per_cu * 256 / BLOCK;  // blocks_per_cu is stated in 256-thread units (4 waves)
  if (cap < 1) cap = 1;
  return cached < cap ? cached : cap;
}

// All launchers are asynchronous on `st`, allocate nothing and never synchronise.
// Grid totals.  Where a launcher hands K integer totals back, its `acc` argument (launch_labels_set: `skipped`) is nullable; when it
// is not NULL it points to K u64 of device memory (launch_correct: kCorrectAccBytes), 8-byte aligned.  The launcher zeroes those
// words on `st`, its kernels add into them (kcommon.hpp: block_accumulate, one atomic per non-zero total and workgroup), and the
// totals are acc[0 .. K - 1] when the launcher's last kernel has run.  The host side of "launch, then read the K totals back" is grid_totals (ctx.hpp).  The passes that keep their acc
// at the front of a run scratch they need anyway (molecules, cells, metrics, launch_feature_filter) say so where they are declared.
hipError_t launch_decode(const LaunchCfg&, const void* recs, size_t n, uint32_t bc_len, uint32_t umi_len,
                         uint8_t* bc, uint8_t* umi, uint64_t* idx, hipStream_t st);
hipError_t launch_encode(const LaunchCfg&, const uint8_t* bc, const uint8_t* umi, const uint64_t* idx,
                         uint64_t first_index, size_t n, uint32_t bc_len, uint32_t umi_len, void* recs,
                         uint64_t* status, hipStream_t st);
hipError_t launch_deserialize(const LaunchCfg&, const void* recs, size_t n, uint64_t* bc, uint64_t* umi,
                              uint64_t* idx, hipStream_t st);
hipError_t launch_serialize(const LaunchCfg&, const uint64_t* bc, const uint64_t* umi, const uint64_t* idx,
                            size_t n, void* recs, hipStream_t st);
hipError_t launch_unpack(const LaunchCfg&, const uint64_t* codes, size_t n, uint32_t len, uint8_t* out,
                         hipStream_t st);
hipError_t launch_pack(const LaunchCfg&, const uint8_t* in, size_t n, uint32_t len, uint64_t* codes,
                       uint64_t* status, hipStream_t st);
static constexpr int kReduceSlots = 64;   // acc: kReduceSlots x 8 u64 (slot 0 after launch_reduce_fold: count, 3 sums, 3 XORs)
static constexpr size_t kReduceAccBytes = (size_t)kReduceSlots * 8 * sizeof(uint64_t);
hipError_t launch_reduce(const LaunchCfg&, const void* recs, size_t n, uint64_t* acc, hipStream_t st);
hipError_t launch_reduce_fold(uint64_t* acc, hipStream_t st);
hipError_t launch_generate(const LaunchCfg&, uint64_t seed, uint64_t first, size_t n, uint32_t bc_len,
                           uint32_t umi_len, void* recs, hipStream_t st);
hipError_t launch_copy(const LaunchCfg&, const void* src, void* dst, size_t bytes, hipStream_t st);
hipError_t launch_sorted_check(const LaunchCfg&, const void* recs, size_t n, uint32_t* flag, hipStream_t st);
hipError_t launch_mismatch(const LaunchCfg&, const void* a, const void* b, size_t nwords, uint64_t* first, hipStream_t st);
hipError_t launch_fill2(uint64_t* p, uint64_t v0, uint64_t v1, hipStream_t st);

// sort.hip
bool trace_sort();   // IBU_TRACE_SORT set to anything but "" / "0" (read once): one stderr line per sort / probed allocation saying what was chosen
hipError_t launch_sort_records(const LaunchCfg&, void* recs, void* tmp, size_t n, void* scratch,
                               size_t scratch_bytes, hipStream_t st, const uint64_t* known_words = nullptr /*u64[6]: OR x 3, AND x 3 of a superset: no census pass*/,
                               int known_prefix = -1 /*>= 0: the 24-byte path's prefix length, estimated elsewhere (0 = all passes)*/);
size_t sort_scratch_bytes(const LaunchCfg&, size_t n);
size_t sort_prefix_estimate_tables(const LaunchCfg&, size_t n);   // bytes of `tables` launch_estimate_prefix_records writes (0: none)
int sort_num_variants();
int sort_num_compact_variants();
hipError_t launch_lower_bound(const void* recs, size_t n, const void* keys, size_t k, uint64_t* pos, hipStream_t st);
// compacted keys (sort.hip): the varying bytes of a set of records as 12-byte elements.  Layout = ibu_key_plan_t (ibu_hip.h).
struct CompactPlan {
  uint32_t csel[4][3];   // compress: element word w = OR over the fields f of perm(f.hi, f.lo, csel[w][f])
  uint32_t xsel[6][2];   // expand: record dword d (= 2 f + half) = base | perm(e.w1, e.w0, xsel[d][0]) | perm(e.w3 or 0, e.w2, xsel[d][1])
  uint32_t k;            // varying bytes (the element bytes above them are zero): 12-byte elements while k <= 12, 16-byte ones (inside the sort) while k <= 16
  uint32_t index_bytes;  // how many of them are index bytes (the least significant element bytes)
  uint64_t base[3];      // each field with its varying bytes cleared (the AND words)
};
void compact_plan_init(const uint64_t or_words[3], const uint64_t and_words[3], CompactPlan* pl);
hipError_t launch_records_census(const LaunchCfg&, const void* recs, size_t n, uint64_t* d_census /*u64[8]*/, hipStream_t st);
hipError_t launch_compact(const LaunchCfg&, const CompactPlan& pl, const void* recs, size_t n, void* elems, hipStream_t st);
hipError_t launch_expand(const LaunchCfg&, const CompactPlan& pl, const void* elems, size_t n, void* recs, hipStream_t st);
// The multi-GPU sort on 12-byte elements (sort.hip, used by multi_sort.cpp): how many prefix passes a sort of n_scale records like
// these n wants (synchronises st); records -> 12-byte elements at `elems`, stamped with their key range among the splitters, -> range order at `out`
// (d_starts: u64[256] in `scratch`, the first element of every range); received elements -> sorted records.
hipError_t launch_estimate_prefix(const LaunchCfg&, const void* recs, size_t n, size_t n_scale, void* tmp, const CompactPlan& pl,
                                  uint32_t* prefix_passes, hipStream_t st);
// The same for the 24-byte path of launch_sort_records (more than 16 varying bytes): the prefix length a sort of n_scale records like
// these n wants (0: all passes), from their census words (OR x 3, AND x 3) alone — what that sort takes as known_prefix.  `tables`:
// sort_prefix_estimate_tables(cfg, n) bytes, 8-byte aligned; no sort scratch is touched.  Synchronises st.
hipError_t launch_estimate_prefix_records(const LaunchCfg&, const void* recs, size_t n, size_t n_scale, const uint64_t words[6], void* tables,
                                          int* prefix_passes, hipStream_t st);
// What the host needs from a partition pass — the range starts (u64[256]) and, where taken, the census words (u64[8]) — exists as soon
// as the pass's small scan kernel has run, BEFORE its scatter kernel (a third of the pass's time) has: with `early` the launcher copies
// both into pinned host memory right there and records `ready` behind the copies, so that the caller can plan the exchange while the
// scatter still runs.
struct PartitionEarly {
  uint64_t* h_starts;   // pinned, u64[256]
  uint64_t* h_words;    // pinned, u64[8] (written only when the census is taken)
  hipEvent_t ready;
};
hipError_t launch_partition_elems(const LaunchCfg&, const CompactPlan& pl, const void* recs, void* elems, size_t n, const void* d_split,
                                  uint32_t nsplit, void* out, void* scratch, size_t scratch_bytes, const uint64_t** d_starts,
                                  const uint64_t** d_census /*nullable: the exact census words of these records, accumulated on the way*/, hipStream_t st,
                                  const PartitionEarly* early = nullptr);
hipError_t launch_records_census_sample(const LaunchCfg&, const void* recs, size_t n, uint64_t* d_census /*u64[8 x 64]*/, bool* exact, hipStream_t st);
hipError_t launch_partition_records(const LaunchCfg&, const void* recs, size_t n, const void* d_split /*24-byte records*/, uint32_t nsplit, void* out,
                                    void* scratch, size_t scratch_bytes, const uint64_t** d_starts,
                                    const uint64_t** d_census /*nullable: the exact OR / AND words of these records, accumulated on the way*/, hipStream_t st,
                                    const PartitionEarly* early = nullptr);   // the same on 24-byte records (any key)
bool sort_elems_supported(const LaunchCfg&, const void* recs, const void* tmp, size_t capacity);
hipError_t launch_sort_elems(const LaunchCfg&, const CompactPlan& pl, void* recs, void* tmp, size_t n, uint32_t prefix_passes, void* scratch,
                             size_t scratch_bytes, hipStream_t st);
// run-length aggregation of sorted records (k_aggregate.hip).  `scratch` holds at least runs_scratch_bytes(n) bytes and is 16-byte aligned.
size_t runs_scratch_bytes(size_t n);
// Barcode: runs of equal w0 with the distinct (w0, w1) ranked inside them; BarcodeStash: the same, and the stash that launch_runs_emit
// at barcode level reads; Pair: runs of equal (w0, w1) with the distinct (w0, w1, w2) ranked inside them.
enum class RunsCount { Barcode, BarcodeStash, Pair };
// The count pass and its scan.  Leaves u64[2] at the front of `scratch`, runs and ranked heads, for the caller to read back, and
// behind them the per-segment tables that the emit pass (or launch_molecules_classify) takes its bases from.
hipError_t launch_runs_count(const LaunchCfg&, const void* recs, size_t n, void* scratch, size_t scratch_bytes, RunsCount what, hipStream_t st);
size_t runs_emit_scratch_bytes(uint64_t n_runs);
// The emit pass on the scratch launch_runs_count left, n_runs and n_ranked being its two totals.  second == NULL: barcode level,
// after RunsCount::BarcodeStash; otherwise pair level, after RunsCount::Pair.  Leaves per run, in ascending key order, first[k]
// (and second[k]) = its first (two) words, counts[k] = its records, distinct[k] (nullable) = the ranked heads in it.  run_scratch
// (runs_emit_scratch_bytes(n_runs) bytes) holds the runs' first rows and ranks in between.
hipError_t launch_runs_emit(const LaunchCfg&, const void* recs, size_t n, const void* scratch, void* run_scratch, uint64_t n_runs,
                            uint64_t n_ranked, uint64_t* first, uint64_t* second, uint64_t* counts, uint64_t* distinct, hipStream_t st);
// Class bytes from the ballots an emit pass left in `scratch` (the count scratch of the same recs and n): record i gets
// verdict[the ordinal of the head it belongs to], ranked heads (ranked: launch_molecules_classify) or run heads (launch_cells_call).
hipError_t launch_class_fill(const LaunchCfg&, const void* recs, size_t n, const void* scratch, bool ranked, const uint8_t* verdict,
                             uint8_t* d_class, hipStream_t st);
// one index per molecule (ibu_classify_molecules, k_molecules.hip).  launch_runs_count(RunsCount::Pair) on a scratch of
// molecules_scratch_bytes(n) comes first; with its second total (the candidates) the caller sizes the run scratch.  Leaves one class
// byte per record in d_class (nullable) and u64[5] at the front of run_scratch: resolved and tied molecules, records of class 0, 1, 2.
size_t molecules_scratch_bytes(size_t n);
size_t molecules_run_scratch_bytes(uint64_t candidates);
hipError_t launch_molecules_classify(const LaunchCfg&, const void* recs, size_t n, void* scratch, void* run_scratch, uint64_t candidates,
                                     bool tie_first, uint8_t* d_class, hipStream_t st);
// cell calling (ibu_call_cells, k_cells.hip).  launch_runs_count(RunsCount::Barcode) on a scratch of cells_scratch_bytes(n) comes
// first; with its two totals (barcodes, pairs) the caller sizes the run scratch.  mode / param: IBU_CELLS_MIN / _TOP / _ORDMAG and
// their parameter (ibu_hip.h).  Leaves one class byte per record in d_class (nullable) and u64[7] at the front of run_scratch: cells,
// reads of cells / of background, umis of cells / of background, threshold, baseline.
size_t cells_scratch_bytes(size_t n);
size_t cells_run_scratch_bytes(uint64_t barcodes);
hipError_t launch_cells_call(const LaunchCfg&, const void* recs, size_t n, void* scratch, void* run_scratch, uint64_t barcodes, uint64_t pairs,
                             uint32_t mode, uint64_t param, bool by_reads, uint8_t* d_class, hipStream_t st);
// The rank-th largest (1 <= rank <= count) of `count` device values below 2^40, by radix selection on the device: leaves it in the
// first u64 of `work` (rank_select_work_bytes() bytes, 8-byte aligned).
size_t rank_select_work_bytes();
hipError_t launch_rank_select(const LaunchCfg&, const uint64_t* values, uint64_t count, uint64_t rank, void* work, hipStream_t st);
// per-barcode QC metrics and the barcode filter (ibu_barcode_metrics, ibu_filter_barcodes, k_metrics.hip).  The feature set: `set`
// (nullable with set_bits == 0) = a device bitmap of set_bits <= 2^32 bits, 8-byte aligned; set_word = 1 or 2, the record word that is
// looked up.  launch_metrics_count on a scratch of metrics_scratch_bytes(n) comes first and leaves u64[5] at its front — barcodes,
// pairs, triples, records in the set, triples in the set; with the first the caller sizes the run scratch.  launch_metrics_table
// writes the columns (each nullable), launch_metrics_filter one class byte per record into d_class (nullable) and u64[10] at the
// front of run_scratch: barcodes per class [4], records per class [4], triples and set triples of class 0.
struct MetricsLimits {   // = ibu_barcode_limits_t (ibu_hip.h)
  uint64_t min_reads, max_reads, min_pairs, max_pairs, min_triples, max_triples, set_num, set_den;
  uint32_t set_of, reserved;
};
// what the launchers (and the C ABI in front of them) accept: set_word 1 or 2, set_bits <= 2^32, a set that is 8-byte aligned and
// non-NULL unless set_bits == 0; set_of 0 or 1 and set_num <= set_den < 2^24
bool metrics_set_ok(const uint64_t* set, uint64_t set_bits, uint32_t set_word);
bool metrics_limits_ok(const MetricsLimits& limits);
size_t metrics_scratch_bytes(size_t n);
size_t metrics_run_scratch_bytes(uint64_t barcodes);
hipError_t launch_metrics_count(const LaunchCfg&, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                                void* scratch, size_t scratch_bytes, hipStream_t st);
hipError_t launch_metrics_table(const LaunchCfg&, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                                const void* scratch, void* run_scratch, uint64_t barcodes, uint64_t* d_barcodes, uint64_t* d_reads,
                                uint64_t* d_pairs, uint64_t* d_triples, uint64_t* d_set_reads, uint64_t* d_set_triples, hipStream_t st);
hipError_t launch_metrics_filter(const LaunchCfg&, const void* recs, size_t n, const uint64_t* set, uint64_t set_bits, uint32_t set_word,
                                 void* scratch, void* run_scratch, uint64_t barcodes, const MetricsLimits& limits, uint8_t* d_class,
                                 hipStream_t st);
// per-feature metrics and the feature filter (ibu_feature_metrics, ibu_filter_features, k_features.hip).  The feature of a record is
// the value of its word feature_word (1 or 2); 1 <= n_features <= 2^32.  launch_feature_count ADDS into the columns (each nullable,
// n_features u64; d_cells only with feature_word 1); its acc (grid totals, u64[4]): reads, umis and cells in range, reads out of
// range.  launch_feature_filter writes the n_features verdict bytes and one class byte per record into d_class (nullable); its `acc`
// is required: kFeatureAccBytes of device memory, 8-byte aligned, zeroed by the launcher, which leaves there the features per
// verdict [0 .. 2] and, with class_totals, the records per class [4 .. 7].
struct FeatureLimits {   // = ibu_feature_limits_t (ibu_hip.h)
  uint64_t min_reads, max_reads, min_umis, max_umis, min_cells, max_cells;
};
static constexpr size_t kFeatureAccBytes = 128;
bool feature_args_ok(uint32_t feature_word, uint64_t n_features);
size_t feature_run_scratch_bytes(uint64_t verdict_bytes);   // acc | a verdict table of that many bytes
hipError_t launch_feature_count(const LaunchCfg&, const void* recs, size_t n, uint32_t feature_word, uint64_t n_features, uint64_t* d_reads,
                                uint64_t* d_umis, uint64_t* d_cells, uint64_t* acc, hipStream_t st);
hipError_t launch_feature_filter(const LaunchCfg&, const void* recs, size_t n, uint32_t feature_word, uint64_t n_features,
                                 const uint64_t* d_reads, const uint64_t* d_umis, const uint64_t* d_cells, const FeatureLimits& limits,
                                 uint8_t* verdict, uint8_t* d_class, bool class_totals, uint64_t* acc, hipStream_t st);
// read subsampling and the saturation curve (ibu_subsample_class, ibu_saturation_curve, k_saturation.hip).  The number of a read is
// splitmix64(base + row) with base = sample_base(seed, first_row); kept at a threshold: ibu_hip.h.
uint64_t sample_base(uint64_t seed, uint64_t first_row);
// One class byte per row into d_class (nullable: the count alone).  acc (grid totals, u64[1]): the number of kept rows.
hipError_t launch_subsample(const LaunchCfg&, size_t n, uint64_t base, uint64_t threshold, uint8_t* d_class, uint64_t* acc, hipStream_t st);
// The curve at k <= kSaturationMaxPoints non-decreasing thresholds (a host array), one read of the records.  Leaves u64[3][32] —
// reads, barcodes, molecules of every point — saturation_points_offset() bytes into `scratch` (saturation_scratch_bytes(n) bytes,
// 16-byte aligned).
static constexpr uint32_t kSaturationMaxPoints = 32;
size_t saturation_scratch_bytes(size_t n);
size_t saturation_points_offset();
hipError_t launch_saturation(const LaunchCfg&, const void* recs, size_t n, uint64_t base, const uint64_t* thresholds, uint32_t k, void* scratch,
                             size_t scratch_bytes, hipStream_t st);
// record i of dst = {w0, w2, w1} of record i of src; dst == src (in place) or disjoint (k_records.hip)
hipError_t launch_swap_fields(const LaunchCfg&, const void* src, void* dst, size_t n, hipStream_t st);
// the stable two-way merge of sorted records (ibu_merge_sorted, ibu_merge_sorted_runs; k_merge.hip).  A wave merges one output tile of
// kMergeTile records.  na, nb > 0 (an empty input is a copy: the caller's); `scratch`: merge_scratch_bytes(na + nb) bytes, 8-byte
// aligned; src (nullable): one byte per output record, 0 = from a, 1 = from b.  out must not overlap a or b.
static constexpr int kMergeTile = 256;
size_t merge_scratch_bytes(size_t n);
hipError_t launch_merge(const LaunchCfg&, const void* a, size_t na, const void* b, size_t nb, void* out, uint8_t* src, void* scratch,
                        hipStream_t st);
// barcode correction against a whitelist (k_whitelist.hip).  The table: `slots` 64-bit keys (a power of two, at least 2 w), all ones =
// free; the all-ones key itself (a legal code at 32 bases) travels beside it as `has_ones`.
struct WhitelistTable { const uint64_t* table; size_t slots; uint32_t bc_len; bool has_ones; };
size_t whitelist_slots(size_t w);
// status: u64[4]; the caller sets [0] to all ones and the rest to 0: [0] lowest position of a code with bits at or above 2*bc_len,
// [1] distinct codes, [2] 1 = the all-ones key is among them.  `table` must be filled with 0xFF bytes.
hipError_t launch_whitelist_build(const LaunchCfg&, const uint64_t* codes, size_t w, uint32_t bc_len, uint64_t* table, size_t slots,
                                  uint64_t* status, hipStream_t st);
// acc (grid totals, u64[4]): the records of class 0 .. 3 — exact, corrected, ambiguous, unmatched.  The one acc that is larger than
// its totals: kCorrectAccBytes, kReduceSlots x 4 u64, which the launcher zeroes and its last kernel folds into the first four words
// (k_whitelist.hip: wl_flush_totals says why).
static constexpr size_t kCorrectAccBytes = (size_t)kReduceSlots * 4 * sizeof(uint64_t);
hipError_t launch_correct(const LaunchCfg&, const WhitelistTable& wl, void* recs, size_t n, uint32_t max_mismatches, uint8_t* d_class,
                          uint64_t* acc, hipStream_t st);
// abundance and resolve (ibu_abundance_add, ibu_abundance_counts, ibu_resolve_barcodes).  counters: wl.slots + 1 u64, one per table
// slot and the last for the all-ones key.  add: d_class nullable (every record counts), otherwise the records whose class c < 8 has
// bit c of class_mask set.  resolve: d_class required; acc (grid totals, u64[4]): examined, resolved, below the share, unseen.
hipError_t launch_abundance_add(const LaunchCfg&, const WhitelistTable& wl, const void* recs, const uint8_t* d_class, size_t n,
                                uint32_t class_mask, uint64_t* counters, hipStream_t st);
hipError_t launch_abundance_counts(const LaunchCfg&, const WhitelistTable& wl, const uint64_t* counters, const uint64_t* codes, size_t k,
                                   uint64_t* out, hipStream_t st);
hipError_t launch_resolve(const LaunchCfg&, const WhitelistTable& wl, const uint64_t* counters, void* recs, size_t n, uint64_t num,
                          uint64_t den, uint8_t* d_class, uint64_t* acc, hipStream_t st);
// labels (ibu_labels_set, ibu_labels_get, ibu_label_records).  labels: wl.slots + 1 bytes, one per table slot and the last for the
// all-ones key.  set: skipped (grid totals, u64[1]): the number of codes skipped.  label_records:
// d_class nullable; acc (nullable): kLabelAccBytes, zeroed by the caller — kReduceSlots x 257 u64, launch_label_fold leaves the 257
// bins (the labels 0 .. 255, then the records not found) in its first 257 words.
static constexpr size_t kLabelAccBytes = (size_t)kReduceSlots * 257 * sizeof(uint64_t);
hipError_t launch_labels_set(const LaunchCfg&, const WhitelistTable& wl, uint8_t* labels, const uint64_t* codes, const uint8_t* vals, size_t k,
                             uint64_t* skipped, hipStream_t st);
hipError_t launch_labels_get(const LaunchCfg&, const WhitelistTable& wl, const uint8_t* labels, const uint64_t* codes, size_t k,
                             uint32_t missing, uint8_t* out, hipStream_t st);
hipError_t launch_label_records(const LaunchCfg&, const WhitelistTable& wl, const uint8_t* labels, const void* recs, size_t n, bool match_mode,
                                uint32_t match, uint32_t missing_class, uint8_t* d_class, uint64_t* acc, hipStream_t st);
hipError_t launch_label_fold(uint64_t* acc, hipStream_t st);
// select: count + scan leave the number of kept records in scratch[0] (u64) and every unit's offset behind it; scatter writes them.
size_t select_scratch_bytes(size_t n);
hipError_t launch_select_count(const LaunchCfg&, const uint8_t* d_class, size_t n, uint32_t keep_mask, void* scratch, size_t scratch_bytes,
                               hipStream_t st);
hipError_t launch_select_scatter(const LaunchCfg&, const void* recs, const uint8_t* d_class, size_t n, uint32_t keep_mask,
                                 const void* scratch, void* out, hipStream_t st);
// partition (ibu_partition_records; k_partition.hip, the plan in partition_plan.hpp): count + scan leave the total in scratch[0] (u64),
// every (part, unit)'s output position behind it and, behind those, the n_parts part starts and the total once more — the n_parts + 1
// words the caller reads back; scatter writes the records.  `map`: the part of every class byte, byte c of the 256 (255 = dropped).
struct PartitionMap { uint32_t w[64]; };
hipError_t launch_partition_count(const LaunchCfg&, const uint8_t* d_class, size_t n, uint32_t n_parts, const PartitionMap& map, void* scratch,
                                  size_t scratch_bytes, hipStream_t st);
hipError_t launch_partition_scatter(const LaunchCfg&, const void* recs, const uint8_t* d_class, size_t n, uint32_t n_parts,
                                    const PartitionMap& map, const void* scratch, void* out, hipStream_t st);
// the matrix export (ibu_matrix_rows, ibu_matrix_market_body; k_matrix.hip), on u64 columns of n entries.  `scratch`:
// matrix_scratch_bytes(n) bytes, 8-byte aligned.  A count launcher (count + scan) leaves u64[4] at its front for the caller to read
// back — [0 .. 2] the largest printed value of each column (text only), [3] the total: rows, or bytes of text — and every unit's
// offset behind them; the scatter / write launcher takes the same scratch.  rows: each output is nullable; row_ptr gets total + 1
// words.  text: `text` at any byte alignment, exactly `total` bytes are written.
size_t matrix_scratch_bytes(size_t n);
static constexpr int kMatrixTotalWord = 3;
hipError_t launch_matrix_rows_count(const LaunchCfg&, const uint64_t* first, size_t n, void* scratch, size_t scratch_bytes, hipStream_t st);
hipError_t launch_matrix_rows_scatter(const LaunchCfg&, const uint64_t* first, size_t n, const void* scratch, uint64_t* row_of_entry,
                                      uint64_t* row_keys, uint64_t* row_ptr, hipStream_t st);
hipError_t launch_matrix_text_count(const LaunchCfg&, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n, uint64_t add_a,
                                    uint64_t add_b, void* scratch, size_t scratch_bytes, hipStream_t st);
hipError_t launch_matrix_text_write(const LaunchCfg&, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n, uint64_t add_a,
                                    uint64_t add_b, const void* scratch, char* text, hipStream_t st);
// the per-row top-2 and the class of a row (ibu_matrix_row_top, ibu_assign_rows; k_matrix.hip).  launch_matrix_row_top runs behind
// launch_matrix_rows_count on the same `scratch`, row_top_scratch_bytes(n) bytes (the scan array, then 88 B per 2048 entries of
// partial tuples): a reduce pass and a finishing pass for the rows that cross a unit seam; each output is nullable and gets one word
// per row; `set` (nullable, then set_bits == 0): the bitmap of ibu_barcode_metrics over the values of `second`.
// launch_matrix_assign: one class byte per row (nullable); acc (grid totals, u64[3]): the rows of class 0, 1, 2; den >= 1 and
// num <= den.
size_t row_top_scratch_bytes(size_t n);
hipError_t launch_matrix_row_top(const LaunchCfg&, const uint64_t* first, const uint64_t* second, const uint64_t* values, size_t n,
                                 const uint64_t* set, uint64_t set_bits, void* scratch, size_t scratch_bytes, uint64_t* top_key,
                                 uint64_t* top_value, uint64_t* next_value, uint64_t* row_sum, uint64_t* row_entries, hipStream_t st);
hipError_t launch_matrix_assign(const LaunchCfg&, const uint64_t* top_value, const uint64_t* next_value, const uint64_t* row_sum, size_t rows,
                                uint64_t min_value, uint64_t num, uint64_t den, uint8_t* d_class, uint64_t* acc, hipStream_t st);

// DEFLATE blocks inflated on the device, one wave per block (k_inflate.hip).  The compressed bytes must be readable 2 KiB past the
// last block (kInflatePad); block i's output goes to d_out_base + ooff (signed: a block that begins in front of the window a batch
// keeps lands in the headroom before it).  d_status[i]: 0 good, 1 not a valid deflate stream of these sizes, 2 CRC-32 mismatch;
// *d_first_bad (the caller sets it to 0xFFFFFFFF): the lowest bad block.
struct InflateBlockDesc { uint64_t coff; int64_t ooff; uint32_t clen, isize, crc, reserved; };
constexpr size_t kInflatePad = 2048;
// form 0: by size; 2: the lanes' tables in scratch whatever the size (k_inflate.hip)
size_t inflate_scratch_bytes(const LaunchCfg&, size_t nblocks, int form = 0);   // the lanes' tables (44 KB per workgroup of the grid; 16 bytes for the LDS form)
hipError_t launch_inflate_blocks(const LaunchCfg&, const void* d_comp, const InflateBlockDesc* d_blocks, size_t nblocks, void* d_out_base,
                                 uint32_t* d_status, uint32_t* d_first_bad, void* scratch, size_t scratch_bytes, hipStream_t st, int form = 0,
                                 const uint64_t* d_ready = nullptr /*the launch runs ahead of its input: compressed bytes arrived so far (status 3: never came)*/,
                                 uint64_t ready_total = 0);

}  // namespace ibu
