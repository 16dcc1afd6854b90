// merge_files — several sorted IBU files (lanes, samples, shards of one run) into one sorted file, without sorting again: every input
// is loaded straight into its slice of ONE device buffer, the slices are the runs of ibu_merge_sorted_runs, and the result is written
// under a header with the sorted flag set (header.rs:111-113).
//   merge_files OUT.ibu IN1.ibu IN2.ibu [...] [--sort-unsorted]
// Inputs may be plain or BGZF (bgzip) files; a BGZF input is inflated on the device (ibu_load_bgzf_to_device).  All headers must agree
// on bc_len and umi_len.  An input whose header does not say sorted is refused — or, with --sort-unsorted, sorted in its slice first
// (ibu_sort_records).  A header that says sorted is taken at its word, as sort_file takes it; the output is checked (ibu_is_sorted).
// Usage errors, unreadable files and header mismatches end the program with a message before any device call.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ibu.hpp"

struct Input {
  std::string path;
  ibu::Header header;
  bool bgzf = false;
  size_t n = 0;          // records
};

// header, compression and record count of one input, on the host
static Input inspect(const std::string& path) {
  Input in;
  in.path = path;
  in.header = ibu::Reader::from_path(path).header();            // through the decompressor where the file is compressed
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  uint64_t payload = bytes.size();
  in.bgzf = bytes.size() >= 2 && bytes[0] == 0x1f && bytes[1] == 0x8b;
  if (in.bgzf) {                                               // the uncompressed size stands in the block trailers
    std::vector<ibu_inflate_block_t> blocks(bytes.size() / 26 + 1);
    size_t n_blocks = 0, consumed = 0;
    ibu::check(ibu_bgzf_scan(bytes.data(), bytes.size(), 1, blocks.data(), blocks.size(), &n_blocks, &consumed, &payload));
  }
  if (payload < ibu::HEADER_SIZE || (payload - ibu::HEADER_SIZE) % ibu::RECORD_SIZE)
    throw std::runtime_error(path + ": not a header and whole records");
  in.n = (payload - ibu::HEADER_SIZE) / ibu::RECORD_SIZE;
  return in;
}

int main(int argc, char** argv) {
  bool sort_unsorted = false, bad = false;
  std::vector<std::string> paths;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--sort-unsorted")) sort_unsorted = true;
    else if (!std::strncmp(argv[i], "--", 2)) bad = true;
    else paths.push_back(argv[i]);
  }
  if (bad || paths.size() < 3) {
    std::fprintf(stderr, "usage: merge_files OUT.ibu IN1.ibu IN2.ibu [...] [--sort-unsorted]\n");
    return 2;
  }
  try {
    using namespace ibu;
    std::vector<Input> inputs;
    size_t total = 0;
    for (size_t i = 1; i < paths.size(); ++i) {
      inputs.push_back(inspect(paths[i]));
      const Input& in = inputs.back();
      const Header& first = inputs.front().header;
      if (in.header.bc_len != first.bc_len || in.header.umi_len != first.umi_len)
        throw std::runtime_error(in.path + ": bc_len / umi_len " + std::to_string(in.header.bc_len) + " / " + std::to_string(in.header.umi_len) +
                                 " differ from " + inputs.front().path + " (" + std::to_string(first.bc_len) + " / " + std::to_string(first.umi_len) + ")");
      if (!in.header.sorted() && !sort_unsorted)
        throw std::runtime_error(in.path + ": the header does not say sorted (--sort-unsorted sorts such an input first)");
      total += in.n;
    }
    // ---- the device from here on
    device::Context ctx(0);
    device::DeviceBuffer recs(ctx, (total ? total : 1) * RECORD_SIZE), tmp(ctx, (total ? total : 1) * RECORD_SIZE);
    std::vector<size_t> runs;
    size_t at = 0;
    for (const Input& in : inputs) {
      void* slice = static_cast<uint8_t*>(recs.ptr()) + at * RECORD_SIZE;
      size_t n = 0;
      if (in.n) {                                              // straight into its slice: d_records given, cap_records = its records
        ibu_header_t h;
        void* p = slice;
        check(in.bgzf ? ibu_load_bgzf_to_device(ctx.raw(), in.path.c_str(), nullptr, &h, &p, in.n, &n, nullptr)
                      : ibu_load_to_device(ctx.raw(), in.path.c_str(), nullptr, &h, &p, in.n, &n, nullptr));
        if (n != in.n || p != slice) throw std::runtime_error(in.path + ": changed while it was read");
        if (!in.header.sorted()) ctx.sort_records(slice, tmp.ptr(), n);
      }
      runs.push_back(n);
      at += n;
    }
    ctx.merge_sorted_runs(recs.ptr(), tmp.ptr(), runs);
    if (total && !ctx.is_sorted(recs.ptr(), total)) throw std::runtime_error("an input claims to be sorted but is not");
    Header out = inputs.front().header;
    out.set_sorted();
    {
      Writer w = Writer::from_path(paths[0], out);
      w.write_batch_device(ctx, recs.ptr(), total);
      w.finish();
    }
    std::printf("%zu records from %zu files -> %s\n", total, inputs.size(), paths[0].c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
