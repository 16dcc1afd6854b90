// demux_file — split a multiplexed records file into one file per sample, in one pass over the records.  A label file says
// which sample every barcode belongs to (the hashtag a cell was assigned, a cluster id); the records are labelled by barcode
// (ibu_label_records), partitioned by label (ibu_partition_records: every sample at once, each in input order) and written as
//   OUT_PREFIX.<label>.ibu
// one file for every label that has reads, each with the input's header — the partition is stable, so a sorted input gives sorted
// files and the sorted flag carries over.
//   demux_file [--missing] IN LABELS.txt OUT_PREFIX
// LABELS.txt: one "barcode label" line per barcode (label: 0 .. 255), as many bases as the file's header says — the format
// count_file --labels reads.  At most 255 distinct labels (254 with --missing).
// --missing: the records whose barcode is not in LABELS.txt go to OUT_PREFIX.missing.ibu, as one more part (without it they are
// dropped).
// One line per file goes to stdout, in the form count_file --label-hist prints:
//   #label<TAB>label<TAB>reads          (the missing file: - for the label)
// The arguments, the label file and the input's header are checked before the device is touched; no output file is created unless
// every device call succeeded.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ibu.hpp"

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
    for (size_t i = 0; i < bc_len; ++i)
      if (!std::strchr("ACGTacgt", line[i])) throw std::runtime_error("the labels file has a barcode with a letter outside ACGT: " + line);
    ascii->insert(ascii->end(), line.begin(), line.begin() + bc_len);
    labels->push_back((uint8_t)label);
  }
  if (labels->empty()) throw std::runtime_error("the labels file is empty");
}

int main(int argc, char** argv) {
  bool missing = false, bad = false;
  for (; argc > 1 && !std::strncmp(argv[1], "--", 2); --argc, ++argv) {
    if (!std::strcmp(argv[1], "--missing")) missing = true;
    else bad = true;
  }
  if (argc != 4 || bad || !argv[3][0]) {
    std::fprintf(stderr, "usage: demux_file [--missing] IN LABELS.txt OUT_PREFIX\n"
                 "       LABELS.txt: one \"barcode label\" line per barcode, label 0 .. 255; writes OUT_PREFIX.<label>.ibu for every label that has reads\n"
                 "       --missing: the records whose barcode is not in LABELS.txt go to OUT_PREFIX.missing.ibu\n");
    return 2;
  }
  const std::string prefix = argv[3];
  try {
    using namespace ibu;
    // the host's checks: the header, the label file, the number of parts
    const Header h = Reader::from_path(argv[1]).header();
    h.validate();
    std::vector<uint8_t> ascii, labels;
    read_labels(argv[2], h.bc_len, &ascii, &labels);
    bool used[256] = {};
    for (uint8_t l : labels) used[l] = true;
    uint8_t part_of[256];
    std::vector<uint32_t> label_of_part;
    for (uint32_t l = 0; l < 256; ++l) {
      part_of[l] = IBU_PART_NONE;
      if (used[l]) label_of_part.push_back(l);
    }
    const size_t most = missing ? 254 : 255;
    if (label_of_part.size() > most)
      throw std::runtime_error("the labels file holds " + std::to_string(label_of_part.size()) + " distinct labels; one call makes " +
                               std::to_string(most) + " files at most" + (missing ? " beside the missing one" : ""));
    uint32_t free_class = 0;                                    // a class byte that is no label: what the records not in the file get
    while (used[free_class]) ++free_class;
    for (size_t p = 0; p < label_of_part.size(); ++p) part_of[label_of_part[p]] = (uint8_t)p;
    uint32_t n_parts = (uint32_t)label_of_part.size();
    if (missing) part_of[free_class] = (uint8_t)n_parts++;

    // the device: load, label, partition once
    device::Context ctx(0);
    auto [h_dev, d_recs, n] = ctx.load_to_device(argv[1]);
    (void)h_dev;
    const size_t w = labels.size();
    std::vector<uint64_t> offsets(n_parts + 1, 0);
    std::vector<Record> out(n);
    if (n) {
      device::DeviceBuffer d_ascii(ctx, ascii.size()), d_codes(ctx, 8 * w), d_labels(ctx, w), d_class(ctx, n), d_out(ctx, n * RECORD_SIZE);
      d_ascii.upload(ascii);
      d_labels.upload(labels);
      ctx.pack_2bit(d_ascii.as<uint8_t>(), w, h.bc_len, d_codes.as<uint64_t>());
      ctx.codec_status();
      device::Whitelist wl(ctx, d_codes.as<uint64_t>(), w, h.bc_len);
      device::Labels lb(ctx, wl);
      lb.set(d_codes.as<uint64_t>(), d_labels.as<uint8_t>(), w);
      ctx.label_records(lb, d_recs, n, d_class.as<uint8_t>(), nullptr, free_class);
      offsets = ctx.partition_records(d_recs, d_class.as<uint8_t>(), n, part_of, n_parts, d_out.ptr(), n);
      ctx.synchronize();
      if (offsets[n_parts]) ctx.download(out.data(), d_out.ptr(), (size_t)offsets[n_parts] * RECORD_SIZE);
    }
    ctx.free(d_recs);

    // the files: every label that has reads, and the missing one when asked for
    for (uint32_t p = 0; p < n_parts; ++p) {
      const bool is_missing = missing && p + 1 == n_parts;
      const size_t lo = (size_t)offsets[p], k = (size_t)(offsets[p + 1] - offsets[p]);
      if (!k && !is_missing) continue;
      const std::string name = is_missing ? std::string("missing") : std::to_string(label_of_part[p]);
      Writer wr = Writer::from_path(prefix + "." + name + ".ibu", h);
      if (k) wr.write_batch(out.data() + lo, k);
      wr.finish();
      std::printf("#label\t%s\t%zu\n", is_missing ? "-" : name.c_str(), k);
    }
    std::fprintf(stderr, "%zu records: %u parts; kept %llu\n", n, n_parts, (unsigned long long)offsets[n_parts]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
