// count_file — the count matrix of a single-cell records file: for every (barcode, index) pair — cell x feature, the index
// word being where users of the format keep the feature number — the number of distinct UMIs (molecules) and of records
// (reads).  Read an IBU file; with a whitelist, correct the barcodes against it (ibu_correct_barcodes) and keep the exact and
// the corrected records (ibu_select_records); build the matrix on the GPU (ibu_count_matrix) and print it in COO form, one
//   barcode<TAB>index<TAB>umis<TAB>reads
// line per entry, ascending by (barcode code, index).  The row lengths of the CSR view — entries per barcode — need nothing
// new: ibu_barcode_counts on the records as ibu_count_matrix leaves them with IBU_COUNT_LEAVE_SWAPPED ({barcode, index, umi})
// returns each barcode and, as its "unique UMIs", its number of distinct indices; they are printed behind the matrix as
//   #row<TAB>barcode<TAB>entries<TAB>reads
//   count_file [--resolve | --resolve=first] [--cells=min:T|top:K|expected:E] [--subsample=F[:seed]] [--saturation=K] IN [WHITELIST.txt]
// WHITELIST.txt: one barcode per line, as many bases as the file's header says.
// --resolve: a (barcode, UMI) molecule seen with several index values counts once, under the index with strictly the most reads, and
// not at all when the top is shared (--resolve=first: under the smallest index at the top) — sort, ibu_classify_molecules,
// ibu_select_records in front of the matrix; the seven totals go to stderr.
// --cells: the matrix of the cells only — sort (unless --resolve already did), ibu_call_cells on the per-barcode UMI counts (min:T a
// fixed minimum, top:K the K largest barcodes and those tied with the last, expected:E a tenth of the 99th percentile of the top
// E), ibu_select_records of the class IBU_CELL; the eight totals go to stderr.
// --subsample=F[:seed]: the matrix of a reproducible random fraction F of the reads (seed: 0 unless given) — behind the last of the
// steps above, on the sorted records (the subset depends on their order): ibu_subsample_class, ibu_select_records of the class
// IBU_SAMPLE_KEPT; the count goes to stderr.
// --saturation=K (1 .. 32): the saturation curve of the records the matrix is counted from, sorted, before their fields are exchanged
// (ibu_saturation_curve, one read of the records), K evenly spaced depths 1/K .. 1, in front of the matrix as
//   #saturation<TAB>fraction<TAB>reads<TAB>barcodes<TAB>molecules<TAB>saturation
// with saturation = 1 - molecules / reads.
//   count_file ... [--qc=minfeat:A[,maxfeat:B][,minumi:C][,maxset:NUM/DEN]] [--set=FILE] IN [WHITELIST.txt]
// --qc: the matrix of the barcodes that pass the per-barcode QC filter — behind the steps above the fields are exchanged and the
// records sorted ONCE by (barcode, index, umi), ibu_filter_barcodes classes every barcode by its features detected (minfeat, maxfeat:
// too few, implausibly many), its UMIs (minumi) and the share of its UMIs whose index is in the set (maxset: above NUM/DEN),
// ibu_select_records keeps the class IBU_BARCODE_PASS, and the matrix and its row lengths are counted from the kept records as they
// stand (ibu_pair_counts, ibu_barcode_counts): no second sort.  The four class totals go to stderr.
// --set=FILE (with --qc): the feature set, one index value per line (mitochondrial genes, spike-ins).
//   count_file ... [--features=mincells:A[,minumi:B][,maxcells:C] --n-features=N] [--feature-table=FILE] IN [WHITELIST.txt]
// --features: the matrix of the features that pass the per-feature filter — behind the cell steps above (--qc included), on the
// records sorted by (barcode, index, umi), ibu_feature_metrics counts for every index value below N its reads, its UMIs and the cells
// it was seen in, ibu_filter_features classes every record by its feature (mincells, maxcells: seen in too few or too many cells;
// minumi: too few UMIs; an index value of N or more is unknown), ibu_select_records keeps the class IBU_FEATURE_PASS, and the matrix
// is counted from the kept records as they stand.  The class totals go to stderr.
// --feature-table=FILE (with --n-features=N): the per-feature table in front of that filter, one
//   index<TAB>reads<TAB>umis<TAB>cells
// line for every index value below N that has a read.
//   count_file ... [--mtx=DIR --n-features=N] IN [WHITELIST.txt]
// --mtx=DIR: the matrix at the end of whatever chain the other options selected, as the directory scanpy's read_10x_mtx and Seurat's
// Read10X read, beside the lines on stdout: DIR/matrix.mtx (MatrixMarket coordinate, features x barcodes, 1-based, the UMI counts),
// DIR/barcodes.tsv and DIR/features.tsv (N lines, the index value as id and name).  The entry table stays on the device:
// ibu_pair_counts into device columns, ibu_matrix_rows numbers the barcodes, ibu_matrix_market_body formats the lines there, and
// the text comes down in pieces.  An index value of N or more is an error, and nothing is written.
//   count_file ... [--assign=min:A[,share:NUM/DEN]] [--set=FILE] IN [WHITELIST.txt]
// --assign: the dominant feature of every barcode — which hashtag, antibody or guide a cell carries — behind whatever chain the other
// options selected, behind the matrix and its rows as one
//   #assign<TAB>barcode<TAB>top_feature<TAB>top<TAB>next<TAB>total<TAB>class
// line per barcode: over the features of --set=FILE (without it: all features) the index value with the most UMIs (the smallest one
// among tied ones; - when the barcode has none of them), its UMIs, the UMIs of the runner-up, the UMIs of all of them, and the class —
// none (fewer than max(A, 1) UMIs at the top), assigned (the top is alone there and holds at least NUM/DEN of the total; without
// share: no such test) or mixed.  ibu_pair_counts into device columns, ibu_matrix_row_top, ibu_assign_rows: the entry table stays on
// the device and 41 bytes per barcode come down.  The four totals go to stderr.
//   count_file ... [--labels=FILE [--keep-label=L] [--label-hist]] IN [WHITELIST.txt]
// --labels=FILE: a per-barcode label table, one "barcode label" line per barcode (label: 0 .. 255) — the hashtag a cell was assigned in
// another library, a cluster id, a QC verdict.  The barcodes become a whitelist of their own and the labels an ibu_labels_t on it.
// --keep-label=L: the matrix of the records whose barcode has label L — ibu_label_records in match mode, ibu_select_records of the
// class IBU_LABEL_IS — behind the whitelist step (the labels then meet corrected barcodes) and in front of whatever chain the other
// options select; the count goes to stderr.
// --label-hist: the reads per label of the records in front of that step (ibu_label_records without class bytes), in front of the matrix as
//   #label<TAB>label<TAB>reads
// one line per label that has a read, and a last one with - for the reads whose barcode is not in FILE.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "ibu.hpp"

static std::string decode(uint64_t code, uint32_t len) {        // base i at bits [2i, 2i+1] (the default base order)
  std::string s(len, 'A');
  for (uint32_t i = 0; i < len; ++i) s[i] = "ACGT"[(code >> (2 * i)) & 3];
  return s;
}

// "min:T" / "top:K" / "expected:E" -> the mode and parameter of ibu_call_cells; false when it is none of them
static bool parse_cells(const char* s, uint32_t* mode, uint64_t* param) {
  static const struct { const char* name; uint32_t mode; } kinds[] = {{"min:", IBU_CELLS_MIN}, {"top:", IBU_CELLS_TOP}, {"expected:", IBU_CELLS_ORDMAG}};
  for (const auto& k : kinds) {
    const size_t len = std::strlen(k.name);
    if (std::strncmp(s, k.name, len)) continue;
    char* end = nullptr;
    if (s[len] < '0' || s[len] > '9') return false;
    *param = std::strtoull(s + len, &end, 10);
    *mode = k.mode;
    return *end == 0 && (k.mode == IBU_CELLS_MIN || *param > 0);
  }
  return false;
}

// "K" -> 1 .. 32 points; false otherwise
static bool parse_saturation(const char* s, uint32_t* k) {
  char* end = nullptr;
  if (s[0] < '0' || s[0] > '9') return false;
  const unsigned long long v = std::strtoull(s, &end, 10);
  *k = (uint32_t)(v <= IBU_SATURATION_MAX_POINTS ? v : 0);
  return *end == 0 && *k >= 1;
}
// "F" or "F:seed" -> a fraction >= 0 and a seed; false otherwise
static bool parse_subsample(const char* s, double* fraction, uint64_t* seed) {
  char* end = nullptr;
  if (!((s[0] >= '0' && s[0] <= '9') || s[0] == '.')) return false;
  *fraction = std::strtod(s, &end);
  *seed = 0;
  if (end == s || !(*fraction >= 0)) return false;
  if (*end == 0) return true;
  if (*end != ':' || end[1] < '0' || end[1] > '9') return false;
  const char* t = end + 1;
  *seed = std::strtoull(t, &end, 10);
  return *end == 0;
}

// "minfeat:A[,maxfeat:B][,minumi:C][,maxset:NUM/DEN]" -> the limits of ibu_filter_barcodes on {barcode, index, umi} records (pairs are
// features, triples UMIs); every key at most once, minfeat among them; false otherwise
static bool parse_qc(const char* s, ibu_barcode_limits_t* lim) {
  *lim = ibu_barcode_limits_t{};
  unsigned seen = 0;
  for (;;) {
    static const char* const keys[] = {"minfeat:", "maxfeat:", "minumi:", "maxset:"};
    unsigned k = 0;
    while (k < 4 && std::strncmp(s, keys[k], std::strlen(keys[k]))) ++k;
    if (k == 4 || (seen >> k & 1)) return false;
    seen |= 1u << k;
    s += std::strlen(keys[k]);
    char* end = nullptr;
    if (*s < '0' || *s > '9') return false;
    errno = 0;
    const uint64_t v = std::strtoull(s, &end, 10);
    if (errno == ERANGE) return false;                         // more than 64 bits
    if (k == 0) lim->min_pairs = v;
    if (k == 1) lim->max_pairs = v;
    if (k == 2) lim->min_triples = v;
    if (k == 3) {
      if (*end != '/' || end[1] < '0' || end[1] > '9') return false;
      lim->set_num = v;
      lim->set_den = std::strtoull(end + 1, &end, 10);
      lim->set_of = 1;                                          // the share of UMIs
      if (errno == ERANGE || lim->set_den == 0 || lim->set_den >= (1ull << 24) || lim->set_num > lim->set_den) return false;
    }
    if (*end == 0) return (seen & 1u) != 0;
    if (*end != ',') return false;
    s = end + 1;
  }
}

// "mincells:A[,minumi:B][,maxcells:C]" -> the limits of ibu_filter_features; every key at most once, mincells among them; false otherwise
static bool parse_features(const char* s, ibu_feature_limits_t* lim) {
  *lim = ibu_feature_limits_t{};
  unsigned seen = 0;
  for (;;) {
    static const char* const keys[] = {"mincells:", "minumi:", "maxcells:"};
    unsigned k = 0;
    while (k < 3 && std::strncmp(s, keys[k], std::strlen(keys[k]))) ++k;
    if (k == 3 || (seen >> k & 1)) return false;
    seen |= 1u << k;
    s += std::strlen(keys[k]);
    char* end = nullptr;
    if (*s < '0' || *s > '9') return false;
    errno = 0;
    const uint64_t v = std::strtoull(s, &end, 10);
    if (errno == ERANGE) return false;                         // more than 64 bits
    if (k == 0) lim->min_cells = v;
    if (k == 1) lim->min_umis = v;
    if (k == 2) lim->max_cells = v;
    if (*end == 0) return (seen & 1u) != 0;
    if (*end != ',') return false;
    s = end + 1;
  }
}
// "N" -> 1 .. 2^32 features; false otherwise
static bool parse_n_features(const char* s, uint64_t* n) {
  char* end = nullptr;
  if (s[0] < '0' || s[0] > '9') return false;
  errno = 0;
  *n = std::strtoull(s, &end, 10);
  return errno != ERANGE && *end == 0 && *n >= 1 && *n <= (1ull << 32);
}

// "min:A[,share:NUM/DEN]" -> the rule of ibu_assign_rows; false otherwise
static bool parse_assign(const char* s, ibu_assign_rule_t* rule) {
  *rule = ibu_assign_rule_t{0, 0, 1};
  char* end = nullptr;
  if (std::strncmp(s, "min:", 4) || s[4] < '0' || s[4] > '9') return false;
  errno = 0;
  rule->min_value = std::strtoull(s + 4, &end, 10);
  if (errno == ERANGE) return false;
  if (*end == 0) return true;
  if (std::strncmp(end, ",share:", 7) || end[7] < '0' || end[7] > '9') return false;
  rule->num = std::strtoull(end + 7, &end, 10);
  if (*end != '/' || end[1] < '0' || end[1] > '9') return false;
  rule->den = std::strtoull(end + 1, &end, 10);
  return errno != ERANGE && *end == 0 && rule->den >= 1 && rule->num <= rule->den;
}

// "L" -> a label 0 .. 255; false otherwise
static bool parse_label(const char* s, uint32_t* label) {
  char* end = nullptr;
  if (s[0] < '0' || s[0] > '9') return false;
  const unsigned long long v = std::strtoull(s, &end, 10);
  *label = (uint32_t)v;
  return *end == 0 && v <= 255;
}
// "barcode label" lines -> the barcodes' text back to back and their labels
static void read_labels(const char* path, uint32_t bc_len, std::vector<uint8_t>* ascii, std::vector<uint8_t>* labels) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  std::string line;
  while (std::getline(f, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    if (line.empty()) continue;
    const size_t gap = line.find_first_of(" \t");
    uint32_t label = 0;
    if (gap != bc_len || !parse_label(line.c_str() + line.find_first_not_of(" \t", gap), &label))
      throw std::runtime_error("the labels file has a line that is not a " + std::to_string(bc_len) + "-base barcode and a label 0 .. 255: " + line);
    ascii->insert(ascii->end(), line.begin(), line.begin() + bc_len);
    labels->push_back((uint8_t)label);
  }
  if (labels->empty()) throw std::runtime_error("the labels file is empty");
}

// one index value per line -> the bitmap of ibu_filter_barcodes and its number of bits (the largest value + 1)
static std::vector<uint64_t> read_set(const char* path, uint64_t* bits) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  std::vector<uint64_t> values;
  std::string line;
  *bits = 0;
  while (std::getline(f, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    if (line.empty()) continue;
    char* end = nullptr;
    errno = 0;
    const uint64_t v = std::strtoull(line.c_str(), &end, 10);
    if (line[0] < '0' || line[0] > '9' || *end != 0) throw std::runtime_error("the set file has a line that is not an index value: " + line);
    if (errno == ERANGE || v >= (1ull << 32)) throw std::runtime_error("the set file has an index value of 2^32 or more: " + line);
    values.push_back(v);
    if (v + 1 > *bits) *bits = v + 1;
  }
  std::vector<uint64_t> words((*bits + 63) / 64 + 1, 0);
  for (uint64_t v : values) words[v >> 6] |= 1ull << (v & 63);
  return words;
}

// --mtx: the 10x directory of the {barcode, index, umi} records as they stand; the entry table never leaves the device as numbers
static void write_mtx(ibu::device::Context& ctx, const void* recs, size_t n, uint32_t bc_len, uint64_t n_features, const std::string& dir) {
  using namespace ibu;
  size_t nnz = 0, rows = 0, bytes = 0;
  check(ibu_pair_counts(ctx.raw(), recs, n, nullptr, nullptr, nullptr, nullptr, 0, &nnz, nullptr, nullptr));
  device::DeviceBuffer d_bc(ctx, 8 * nnz), d_idx(ctx, 8 * nnz), d_reads(ctx, 8 * nnz), d_umis(ctx, 8 * nnz), d_ord(ctx, 8 * nnz);
  check(ibu_pair_counts(ctx.raw(), recs, n, d_bc.as<uint64_t>(), d_idx.as<uint64_t>(), d_reads.as<uint64_t>(), d_umis.as<uint64_t>(), nnz, &nnz,
                        nullptr, nullptr));
  rows = ctx.matrix_rows(d_bc.as<uint64_t>(), nnz, nullptr, nullptr, nullptr, 0);
  device::DeviceBuffer d_keys(ctx, 8 * rows), d_ascii(ctx, (size_t)bc_len * rows);
  ctx.matrix_rows(d_bc.as<uint64_t>(), nnz, d_ord.as<uint64_t>(), d_keys.as<uint64_t>(), nullptr, rows);
  // the size query on the values as they stand says what the largest index is; adding one lengthens a line by at most two bytes
  uint64_t maxima[3] = {0, 0, 0};
  bytes = ctx.matrix_market_body(d_idx.as<uint64_t>(), d_ord.as<uint64_t>(), d_umis.as<uint64_t>(), nnz, nullptr, 0, 0, 0, maxima);
  if (nnz && maxima[0] >= n_features)
    throw std::runtime_error("--mtx: the records hold index " + std::to_string(maxima[0]) + ", which is not below --n-features");
  const size_t cap = bytes + 2 * nnz;
  device::DeviceBuffer d_text(ctx, cap);
  bytes = ctx.matrix_market_body(d_idx.as<uint64_t>(), d_ord.as<uint64_t>(), d_umis.as<uint64_t>(), nnz, d_text.as<char>(), cap, 1, 1);
  ctx.unpack_2bit(d_keys.as<uint64_t>(), rows, bc_len, d_ascii.as<uint8_t>());
  ctx.synchronize();
  const auto open = [&](const char* name) {
    std::FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + dir + "/" + name + " (the directory must exist)");
    return f;
  };
  const auto close = [&](std::FILE* f, const char* name) {
    if (std::fclose(f)) throw std::runtime_error("cannot write " + dir + "/" + name);
  };
  std::FILE* f = open("matrix.mtx");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate integer general\n%llu %zu %zu\n", (unsigned long long)n_features, rows, nnz);
  std::vector<char> piece(std::min<size_t>(bytes, (size_t)64 << 20));
  for (size_t off = 0; off < bytes; off += piece.size()) {
    const size_t k = std::min(piece.size(), bytes - off);
    ctx.download(piece.data(), d_text.as<char>() + off, k);
    std::fwrite(piece.data(), 1, k, f);
  }
  close(f, "matrix.mtx");
  f = open("barcodes.tsv");
  const std::vector<uint8_t> ascii = d_ascii.download<uint8_t>((size_t)bc_len * rows);
  for (size_t r = 0; r < rows; ++r) {
    std::fwrite(ascii.data() + r * bc_len, 1, bc_len, f);
    std::fputc('\n', f);
  }
  close(f, "barcodes.tsv");
  f = open("features.tsv");
  for (uint64_t j = 0; j < n_features; ++j) std::fprintf(f, "%llu\t%llu\tGene Expression\n", (unsigned long long)j, (unsigned long long)j);
  close(f, "features.tsv");
}

// --assign: one line per barcode of the {barcode, index, umi} records as they stand, and the totals
static void print_assignment(ibu::device::Context& ctx, const void* recs, size_t n, uint32_t bc_len, const ibu_assign_rule_t& rule,
                             const char* set_path) {
  using namespace ibu;
  uint64_t set_bits = 0;
  std::vector<uint64_t> words(1, 0);
  if (set_path) words = read_set(set_path, &set_bits);
  device::DeviceBuffer d_set(ctx, 8 * words.size());
  d_set.upload(words);
  const uint64_t* set = set_path ? d_set.as<uint64_t>() : nullptr;   // an empty file is the empty set, not "all features"
  size_t nnz = 0;
  check(ibu_pair_counts(ctx.raw(), recs, n, nullptr, nullptr, nullptr, nullptr, 0, &nnz, nullptr, nullptr));
  device::DeviceBuffer d_bc(ctx, 8 * nnz), d_idx(ctx, 8 * nnz), d_reads(ctx, 8 * nnz), d_umis(ctx, 8 * nnz);
  check(ibu_pair_counts(ctx.raw(), recs, n, d_bc.as<uint64_t>(), d_idx.as<uint64_t>(), d_reads.as<uint64_t>(), d_umis.as<uint64_t>(), nnz, &nnz,
                        nullptr, nullptr));
  const size_t rows = ctx.matrix_rows(d_bc.as<uint64_t>(), nnz, nullptr, nullptr, nullptr, 0);
  device::DeviceBuffer d_keys(ctx, 8 * rows), d_key(ctx, 8 * rows), d_top(ctx, 8 * rows), d_next(ctx, 8 * rows), d_sum(ctx, 8 * rows), d_class(ctx, rows);
  ctx.matrix_rows(d_bc.as<uint64_t>(), nnz, nullptr, d_keys.as<uint64_t>(), nullptr, rows);
  ctx.matrix_row_top(d_bc.as<uint64_t>(), d_idx.as<uint64_t>(), d_umis.as<uint64_t>(), nnz,
                     {d_key.as<uint64_t>(), d_top.as<uint64_t>(), d_next.as<uint64_t>(), d_sum.as<uint64_t>(), nullptr}, rows, set, set_bits);
  const device::AssignCounts c = ctx.assign_rows(d_top.as<uint64_t>(), d_next.as<uint64_t>(), d_sum.as<uint64_t>(), rows, rule, d_class.as<uint8_t>());
  const auto bc = d_keys.download<uint64_t>(rows), key = d_key.download<uint64_t>(rows), top = d_top.download<uint64_t>(rows),
             next = d_next.download<uint64_t>(rows), sum = d_sum.download<uint64_t>(rows);
  const auto cls = d_class.download<uint8_t>(rows);
  static const char* const names[] = {"assigned", "none", "mixed"};
  for (size_t r = 0; r < rows; ++r) {
    const std::string feature = key[r] == IBU_NO_KEY ? "-" : std::to_string(key[r]);
    std::printf("#assign\t%s\t%s\t%llu\t%llu\t%llu\t%s\n", decode(bc[r], bc_len).c_str(), feature.c_str(), (unsigned long long)top[r],
                (unsigned long long)next[r], (unsigned long long)sum[r], cls[r] < 3 ? names[cls[r]] : "?");
  }
  std::fprintf(stderr, "%zu barcodes: assigned %llu, none %llu, mixed %llu\n", (size_t)c.rows, (unsigned long long)c.assigned,
               (unsigned long long)c.none, (unsigned long long)c.mixed);
}

int main(int argc, char** argv) {
  int resolve = 0;                                              // 1: --resolve, 2: --resolve=first
  bool cells = false, bad = false, subsample = false, qc = false, features = false, assign = false, keep_label = false, label_hist = false;
  const char* labels_path = nullptr;
  uint32_t kept_label = 0;
  ibu_assign_rule_t assign_rule{0, 0, 1};
  ibu_barcode_limits_t qc_limits{};
  ibu_feature_limits_t feature_limits{};
  uint64_t n_features = 0;
  const char* set_path = nullptr;
  const char* table_path = nullptr;
  const char* mtx_dir = nullptr;
  uint32_t cells_mode = 0, saturation = 0;
  uint64_t cells_param = 0, sample_seed = 0;
  double sample_fraction = 1;
  for (; argc > 1 && !std::strncmp(argv[1], "--", 2); --argc, ++argv) {
    if (!std::strcmp(argv[1], "--resolve")) resolve = 1;
    else if (!std::strcmp(argv[1], "--resolve=first")) resolve = 2;
    else if (!std::strncmp(argv[1], "--cells=", 8) && parse_cells(argv[1] + 8, &cells_mode, &cells_param)) cells = true;
    else if (!std::strncmp(argv[1], "--subsample=", 12) && parse_subsample(argv[1] + 12, &sample_fraction, &sample_seed)) subsample = true;
    else if (!std::strncmp(argv[1], "--saturation=", 13) && parse_saturation(argv[1] + 13, &saturation)) {}
    else if (!std::strncmp(argv[1], "--qc=", 5) && parse_qc(argv[1] + 5, &qc_limits)) qc = true;
    else if (!std::strncmp(argv[1], "--set=", 6) && argv[1][6]) set_path = argv[1] + 6;
    else if (!std::strncmp(argv[1], "--features=", 11) && parse_features(argv[1] + 11, &feature_limits)) features = true;
    else if (!std::strncmp(argv[1], "--n-features=", 13) && parse_n_features(argv[1] + 13, &n_features)) {}
    else if (!std::strncmp(argv[1], "--feature-table=", 16) && argv[1][16]) table_path = argv[1] + 16;
    else if (!std::strncmp(argv[1], "--mtx=", 6) && argv[1][6]) mtx_dir = argv[1] + 6;
    else if (!std::strncmp(argv[1], "--assign=", 9) && parse_assign(argv[1] + 9, &assign_rule)) assign = true;
    else if (!std::strncmp(argv[1], "--labels=", 9) && argv[1][9]) labels_path = argv[1] + 9;
    else if (!std::strncmp(argv[1], "--keep-label=", 13) && parse_label(argv[1] + 13, &kept_label)) keep_label = true;
    else if (!std::strcmp(argv[1], "--label-hist")) label_hist = true;
    else bad = true;
  }
  const bool feature_steps = features || table_path;            // --mtx wants N as well, and none of the feature steps
  if (argc < 2 || bad || (set_path && !qc && !assign) || ((feature_steps || mtx_dir) != (n_features != 0)) ||
      ((keep_label || label_hist) && !labels_path)) {
    std::fprintf(stderr, "usage: count_file [--resolve | --resolve=first] [--cells=min:T|top:K|expected:E] [--subsample=F[:seed]] [--saturation=K] "
                 "IN [WHITELIST.txt]\n"
                 "       further options: [--qc=minfeat:A[,maxfeat:B][,minumi:C][,maxset:NUM/DEN]] [--set=FILE] (FILE: one index value per line)\n"
                 "                        [--features=mincells:A[,minumi:B][,maxcells:C] --n-features=N] [--feature-table=FILE] (with --n-features=N)\n"
                 "                        [--mtx=DIR --n-features=N] (matrix.mtx, barcodes.tsv, features.tsv)\n"
                 "                        [--assign=min:A[,share:NUM/DEN]] [--set=FILE] (the dominant feature of every barcode, over the set)\n"
                 "                        [--labels=FILE [--keep-label=L] [--label-hist]] (FILE: one \"barcode label\" line per barcode, label 0 .. 255)\n");
    return 2;
  }
  try {
    using namespace ibu;
    device::Context ctx(0);
    auto [h, d_recs, n] = ctx.load_to_device(argv[1]);          // load_to_vec, device form
    device::DeviceBuffer tmp(ctx, (n ? n : 1) * RECORD_SIZE);
    void* recs = d_recs;                                        // the records the matrix is built from, and its scratch
    void* scratch = tmp.ptr();
    size_t kept = n;
    if (argc > 2 && n) {
      std::vector<uint8_t> ascii;
      size_t w = 0;
      std::ifstream f(argv[2]);
      if (!f) throw std::runtime_error(std::string("cannot open ") + argv[2]);
      std::string line;
      while (std::getline(f, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        if (line.size() != h.bc_len) throw std::runtime_error("whitelist line " + std::to_string(w + 1) + " is not " + std::to_string(h.bc_len) + " bases long");
        ascii.insert(ascii.end(), line.begin(), line.end());
        ++w;
      }
      if (!w) throw std::runtime_error("the whitelist is empty");
      device::DeviceBuffer d_ascii(ctx, ascii.size()), d_codes(ctx, 8 * w), d_class(ctx, n);
      d_ascii.upload(ascii);
      ctx.pack_2bit(d_ascii.as<uint8_t>(), w, h.bc_len, d_codes.as<uint64_t>());
      ctx.codec_status();                                       // throws InvalidBase on a letter outside ACGTacgt
      device::Whitelist wl(ctx, d_codes.as<uint64_t>(), w, h.bc_len);
      const device::CorrectCounts c = ctx.correct_barcodes(wl, d_recs, n, 1, d_class.as<uint8_t>());
      kept = ctx.select_records(d_recs, d_class.as<uint8_t>(), n, 0b0011, tmp.ptr(), n);
      ctx.synchronize();
      std::fprintf(stderr, "%zu records: exact %llu, corrected %llu, ambiguous %llu, unmatched %llu; kept %zu\n", n, (unsigned long long)c.exact,
                   (unsigned long long)c.corrected, (unsigned long long)c.ambiguous, (unsigned long long)c.unmatched, kept);
      recs = tmp.ptr();                                         // the kept records live in tmp; the input array is scratch from here on
      scratch = d_recs;
    }
    if (labels_path && !kept && label_hist) std::printf("#label\t-\t0\n");   // no record: no label has a read, and none is missing
    if (labels_path && kept) {                                  // a label per barcode -> reads per label, and the records of one label
      std::vector<uint8_t> ascii, labels;
      read_labels(labels_path, h.bc_len, &ascii, &labels);
      const size_t w = labels.size();
      device::DeviceBuffer d_ascii(ctx, ascii.size()), d_codes(ctx, 8 * w), d_labels(ctx, w);
      d_ascii.upload(ascii);
      d_labels.upload(labels);
      ctx.pack_2bit(d_ascii.as<uint8_t>(), w, h.bc_len, d_codes.as<uint64_t>());
      ctx.codec_status();                                       // throws InvalidBase on a letter outside ACGTacgt
      device::Whitelist cells_wl(ctx, d_codes.as<uint64_t>(), w, h.bc_len);
      device::Labels lb(ctx, cells_wl);
      lb.set(d_codes.as<uint64_t>(), d_labels.as<uint8_t>(), w);
      if (label_hist) {
        uint64_t hist[IBU_LABEL_BINS];
        ctx.label_records(lb, recs, kept, nullptr, hist);
        for (uint32_t l = 0; l < 256; ++l)
          if (hist[l]) std::printf("#label\t%u\t%llu\n", l, (unsigned long long)hist[l]);
        std::printf("#label\t-\t%llu\n", (unsigned long long)hist[256]);
      }
      if (keep_label) {
        device::DeviceBuffer d_class(ctx, kept);
        const size_t before = kept;
        ctx.label_records_match(lb, recs, before, kept_label, d_class.as<uint8_t>());
        kept = ctx.select_records(recs, d_class.as<uint8_t>(), before, 1u << IBU_LABEL_IS, scratch, before);
        ctx.synchronize();
        std::fprintf(stderr, "%zu records: label %u; kept %zu\n", before, kept_label, kept);
        std::swap(recs, scratch);
      }
    }
    if (resolve && kept) {                                      // sort -> classify -> keep class 0: one index per molecule
      ctx.sort_records(recs, scratch, kept);
      device::DeviceBuffer d_class(ctx, kept);
      const device::MoleculeCounts m = ctx.classify_molecules(recs, kept, d_class.as<uint8_t>(), resolve == 2);
      const size_t before = kept;
      kept = ctx.select_records(recs, d_class.as<uint8_t>(), before, 1u << IBU_MOLECULE_KEPT, scratch, before);
      ctx.synchronize();
      std::fprintf(stderr, "%zu records: molecules %llu, candidates %llu, resolved %llu, tied %llu; reads kept %llu, minor %llu, tied %llu\n", before,
                   (unsigned long long)m.molecules, (unsigned long long)m.candidates, (unsigned long long)m.resolved, (unsigned long long)m.tied,
                   (unsigned long long)m.reads_kept, (unsigned long long)m.reads_minor, (unsigned long long)m.reads_tied);
      std::swap(recs, scratch);
    }
    if (cells && kept) {                                        // sorted records -> the class of every barcode -> the records of the cells
      if (!resolve) ctx.sort_records(recs, scratch, kept);
      device::DeviceBuffer d_class(ctx, kept);
      const device::CellCounts c = ctx.call_cells(recs, kept, cells_mode, cells_param, d_class.as<uint8_t>());
      const size_t before = kept;
      kept = ctx.select_records(recs, d_class.as<uint8_t>(), before, 1u << IBU_CELL, scratch, before);
      ctx.synchronize();
      std::fprintf(stderr, "%zu records: barcodes %llu, cells %llu, threshold %llu, baseline %llu; reads of cells %llu, of background %llu; "
                   "umis of cells %llu, of background %llu\n", before, (unsigned long long)c.barcodes, (unsigned long long)c.cells,
                   (unsigned long long)c.threshold, (unsigned long long)c.baseline, (unsigned long long)c.reads_cells,
                   (unsigned long long)c.reads_background, (unsigned long long)c.umis_cells, (unsigned long long)c.umis_background);
      std::swap(recs, scratch);
    }
    bool sorted = (resolve || cells) && kept;                   // (ibu_select_records keeps the order)
    if (subsample && kept) {                                    // sorted records -> a class per row -> the kept reads
      if (!sorted) ctx.sort_records(recs, scratch, kept);
      sorted = true;
      device::DeviceBuffer d_class(ctx, kept);
      const size_t before = kept;
      ctx.subsample_class_async(before, device::Context::sample_threshold(sample_fraction), d_class.as<uint8_t>(), sample_seed);
      kept = ctx.select_records(recs, d_class.as<uint8_t>(), before, 1u << IBU_SAMPLE_KEPT, scratch, before);
      ctx.synchronize();
      std::fprintf(stderr, "%zu records: subsample %g seed %llu; kept %zu\n", before, sample_fraction, (unsigned long long)sample_seed, kept);
      std::swap(recs, scratch);
    }
    if (saturation) {                                           // K depths from one read of the sorted records
      if (!sorted && kept) ctx.sort_records(recs, scratch, kept);
      std::vector<uint64_t> thresholds(saturation);
      for (uint32_t j = 1; j <= saturation; ++j)                // the floor of (j / K) 2^64; j == K: everything
        thresholds[j - 1] = j == saturation ? UINT64_MAX : (uint64_t)((((unsigned __int128)j) << 64) / saturation);
      const auto curve = ctx.saturation_curve(recs, kept, thresholds);
      for (uint32_t j = 0; j < saturation; ++j) {
        const device::SaturationPoint& p = curve[j];
        std::printf("#saturation\t%.6f\t%llu\t%llu\t%llu\t%.6f\n", (double)(j + 1) / saturation, (unsigned long long)p.reads,
                    (unsigned long long)p.barcodes, (unsigned long long)p.molecules, p.reads ? 1.0 - (double)p.molecules / (double)p.reads : 0.0);
      }
    }
    // the matrix; the records stay {barcode, index, umi} so that the row lengths can be read off them
    std::vector<device::MatrixEntry> entries;
    if (qc) {                                                   // exchange, sort once, class every barcode, keep the passing ones, count them as they stand
      uint64_t set_bits = 0;
      std::vector<uint64_t> words(1, 0);
      if (set_path) words = read_set(set_path, &set_bits);
      device::DeviceBuffer d_set(ctx, 8 * words.size()), d_class(ctx, kept ? kept : 1);
      d_set.upload(words);
      ctx.swap_umi_index(recs, recs, kept);
      if (kept) ctx.sort_records(recs, scratch, kept);
      const size_t before = kept;
      const device::BarcodeFilterCounts c =
          ctx.filter_barcodes(recs, before, {set_bits ? d_set.as<uint64_t>() : nullptr, set_bits}, 1, qc_limits, d_class.as<uint8_t>());
      if (before) kept = ctx.select_records(recs, d_class.as<uint8_t>(), before, 1u << IBU_BARCODE_PASS, scratch, before);
      ctx.synchronize();
      std::fprintf(stderr, "%zu records: barcodes %llu: pass %llu, low %llu, high %llu, set %llu; reads pass %llu, low %llu, high %llu, set %llu\n", before,
                   (unsigned long long)c.barcodes, (unsigned long long)c.barcodes_by_class[0], (unsigned long long)c.barcodes_by_class[1],
                   (unsigned long long)c.barcodes_by_class[2], (unsigned long long)c.barcodes_by_class[3], (unsigned long long)c.reads_by_class[0],
                   (unsigned long long)c.reads_by_class[1], (unsigned long long)c.reads_by_class[2], (unsigned long long)c.reads_by_class[3]);
      std::swap(recs, scratch);
    } else if (feature_steps) {                                 // the feature steps want the same order
      ctx.swap_umi_index(recs, recs, kept);
      if (kept) ctx.sort_records(recs, scratch, kept);
    }
    if (feature_steps) {                                        // count every feature, class every record by its feature, keep the passing ones
      device::DeviceBuffer d_reads(ctx, 8 * n_features), d_umis(ctx, 8 * n_features), d_cells(ctx, 8 * n_features);
      const device::FeatureTotals t = ctx.feature_metrics(recs, kept, n_features, d_reads.as<uint64_t>(), d_umis.as<uint64_t>(), d_cells.as<uint64_t>());
      std::fprintf(stderr, "%zu records: %llu features: reads %llu, umis %llu, cells %llu; reads of other index values %llu\n", kept,
                   (unsigned long long)n_features, (unsigned long long)t.reads, (unsigned long long)t.umis, (unsigned long long)t.cells,
                   (unsigned long long)t.reads_out_of_range);
      if (table_path) {
        const auto hr = d_reads.download<uint64_t>(n_features), hu = d_umis.download<uint64_t>(n_features), hc = d_cells.download<uint64_t>(n_features);
        std::FILE* f = std::fopen(table_path, "w");
        if (!f) throw std::runtime_error(std::string("cannot write ") + table_path);
        for (uint64_t k = 0; k < n_features; ++k)
          if (hr[k]) std::fprintf(f, "%llu\t%llu\t%llu\t%llu\n", (unsigned long long)k, (unsigned long long)hr[k], (unsigned long long)hu[k], (unsigned long long)hc[k]);
        if (std::fclose(f)) throw std::runtime_error(std::string("cannot write ") + table_path);
      }
      if (features) {
        device::DeviceBuffer d_class(ctx, kept ? kept : 1);
        const size_t before = kept;
        const device::FeatureFilterCounts c = ctx.filter_features(recs, before, n_features, d_reads.as<uint64_t>(), d_umis.as<uint64_t>(),
                                                                  d_cells.as<uint64_t>(), feature_limits, d_class.as<uint8_t>());
        if (before) kept = ctx.select_records(recs, d_class.as<uint8_t>(), before, 1u << IBU_FEATURE_PASS, scratch, before);
        ctx.synchronize();
        std::fprintf(stderr, "%zu records: features pass %llu, low %llu, high %llu; reads pass %llu, low %llu, high %llu, unknown %llu\n", before,
                     (unsigned long long)c.features_by_class[0], (unsigned long long)c.features_by_class[1], (unsigned long long)c.features_by_class[2],
                     (unsigned long long)c.reads_by_class[0], (unsigned long long)c.reads_by_class[1], (unsigned long long)c.reads_by_class[2],
                     (unsigned long long)c.reads_by_class[3]);
        std::swap(recs, scratch);
      }
    }
    if (qc || feature_steps) entries = ctx.pair_counts(recs, kept);   // the records are sorted by (barcode, index, umi) already
    else entries = ctx.count_matrix(recs, scratch, kept, 0, /*leave_swapped=*/true);
    for (const device::MatrixEntry& e : entries)
      std::printf("%s\t%llu\t%llu\t%llu\n", decode(e.first, h.bc_len).c_str(), (unsigned long long)e.second, (unsigned long long)e.distinct,
                  (unsigned long long)e.records);
    size_t total = 0;
    for (auto& [barcode, reads, n_entries] : ctx.barcode_counts(recs, kept)) {
      std::printf("#row\t%s\t%llu\t%llu\n", decode(barcode, h.bc_len).c_str(), (unsigned long long)n_entries, (unsigned long long)reads);
      total += n_entries;
    }
    if (total != entries.size()) throw std::runtime_error("the row lengths do not add up to the number of entries");
    if (mtx_dir) write_mtx(ctx, recs, kept, h.bc_len, n_features, mtx_dir);
    if (assign) print_assignment(ctx, recs, kept, h.bc_len, assign_rule, set_path);
    ctx.free(d_recs);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
