// correct_file — barcodes as they come off a sequencer carry substitution errors; the standard first step of an analysis
// moves every barcode that has exactly one whitelist entry one substitution away onto that entry and drops what matches
// nothing.  Read an IBU file, correct its barcodes against a whitelist on the GPU (ibu_correct_barcodes), keep the exact and
// the corrected records (ibu_select_records), sort them and write them under a header with the sorted flag set.
//   correct_file IN WHITELIST.txt OUT [--keep-ambiguous] [--resolve[=NUM/DEN]]
// WHITELIST.txt: one barcode per line, as many bases as the file's header says.  --keep-ambiguous: records with two or more
// whitelist entries at distance one stay too (uncorrected).  --resolve: such a record moves onto the candidate that holds at least
// NUM/DEN (default 39/40) of the exactly matching reads among its candidates (ibu_abundance_add over the exact records, then
// ibu_resolve_barcodes) and is kept; where no candidate does, it is dropped as before.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ibu.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: correct_file IN WHITELIST.txt OUT [--keep-ambiguous] [--resolve[=NUM/DEN]]\n"); return 2; }
  uint32_t keep = 0b0011;                                       // classes 0 (exact) and 1 (corrected)
  bool resolve = false;
  unsigned long long num = 39, den = 40;
  for (int i = 4; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--keep-ambiguous")) keep |= 0b0100;
    if (!std::strncmp(argv[i], "--resolve", 9) && (argv[i][9] == 0 || argv[i][9] == '=')) {
      resolve = true;
      keep |= 1u << IBU_BARCODE_RESOLVED;
      if (argv[i][9] == '=' && std::sscanf(argv[i] + 10, "%llu/%llu", &num, &den) != 2) {
        std::fprintf(stderr, "--resolve=NUM/DEN: two integers, e.g. --resolve=39/40\n");
        return 2;
      }
    }
  }
  try {
    using namespace ibu;
    device::Context ctx(0);
    auto [h, d_recs, n] = ctx.load_to_device(argv[1]);          // load_to_vec, device form
    // the whitelist: text -> one ASCII column -> 2-bit codes on the device (the codec's own pack)
    std::vector<uint8_t> ascii;
    size_t w = 0;
    {
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
    }
    if (!w) throw std::runtime_error("the whitelist is empty");
    device::DeviceBuffer d_ascii(ctx, ascii.size()), d_codes(ctx, 8 * w);
    d_ascii.upload(ascii);
    ctx.pack_2bit(d_ascii.as<uint8_t>(), w, h.bc_len, d_codes.as<uint64_t>());
    ctx.codec_status();                                         // throws InvalidBase on a letter outside ACGTacgt
    device::Whitelist wl(ctx, d_codes.as<uint64_t>(), w, h.bc_len);

    device::DeviceBuffer tmp(ctx, n * RECORD_SIZE), d_class(ctx, n);
    // how many barcodes the file has as it stands (the sort does not change what is corrected)
    ctx.sort_records(d_recs, tmp.ptr(), n);
    const size_t before = ctx.barcode_counts(d_recs, n).size();
    const device::CorrectCounts c = ctx.correct_barcodes(wl, d_recs, n, 1, d_class.as<uint8_t>());
    device::ResolveCounts r{};
    if (resolve) {
      device::Abundance ab(ctx, wl);
      ab.add(d_recs, n, d_class.as<uint8_t>(), 1u << 0);        // the prior: the exactly matching reads of every whitelist entry
      r = ctx.resolve_barcodes(wl, ab, d_recs, n, d_class.as<uint8_t>(), num, den);
    }
    const size_t kept = ctx.select_records(d_recs, d_class.as<uint8_t>(), n, keep, tmp.ptr(), n);
    ctx.sort_records(tmp.ptr(), d_recs, kept);                  // the input array is scratch from here on
    const size_t after = ctx.barcode_counts(tmp.ptr(), kept).size();
    Header out = h;
    out.set_sorted();
    {
      Writer wr = Writer::from_path(argv[3], out);
      wr.write_batch_device(ctx, tmp.ptr(), kept);
      wr.finish();
    }
    ctx.free(d_recs);
    std::printf("%zu records, whitelist of %zu (%zu distinct): exact %llu, corrected %llu, ambiguous %llu, unmatched %llu; kept %zu\n", n, w,
                wl.n_distinct(), (unsigned long long)c.exact, (unsigned long long)c.corrected, (unsigned long long)c.ambiguous,
                (unsigned long long)c.unmatched, kept);
    if (resolve)
      std::printf("ambiguous examined %llu: resolved %llu at a share of %llu/%llu, below the share %llu, no exact read among the candidates %llu\n",
                  (unsigned long long)r.examined, (unsigned long long)r.resolved, num, den, (unsigned long long)r.below_share,
                  (unsigned long long)r.unseen);
    std::printf("barcodes before %zu, after %zu\n", before, after);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
