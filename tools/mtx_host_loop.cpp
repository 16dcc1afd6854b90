// mtx_host_loop — the yardstick of tools/aggbench.py --mtx: the loop examples/count_file.cpp prints its matrix with, one printf per
// entry on one host thread, over downloaded columns.  Built by the tool into a shared object and called through ctypes; returns the
// wall time of the loop in seconds (the file is opened before the clock starts and closed after it stops), or -1 if `path` cannot
// be written.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>

static std::string decode(uint64_t code, uint32_t len) {        // as count_file.cpp: base i at bits [2i, 2i+1]
  std::string s(len, 'A');
  for (uint32_t i = 0; i < len; ++i) s[i] = "ACGT"[(code >> (2 * i)) & 3];
  return s;
}

extern "C" double mtx_host_loop(const uint64_t* barcodes, const uint64_t* indices, const uint64_t* umis, const uint64_t* reads, size_t n,
                                uint32_t bc_len, const char* path) {
  std::FILE* f = std::fopen(path, "w");
  if (!f) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t k = 0; k < n; ++k)
    std::fprintf(f, "%s\t%llu\t%llu\t%llu\n", decode(barcodes[k], bc_len).c_str(), (unsigned long long)indices[k], (unsigned long long)umis[k],
                 (unsigned long long)reads[k]);
  std::fflush(f);
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::fclose(f);
  return s;
}
