// TEST INFRASTRUCTURE: a stand-alone program over the engine + kernels compiled for the CPU lane emulator (as
// tests/emu/tbz_emu.cpp compiles them), built with AddressSanitizer + UBSan by tests/test_search_san.py.
//   search_san_main <stream> <format 0..2> <delim> <spacing> <queries> <out>
// reads a compressed stream and a list of queries ("first count max_hits pattern-in-hex" per line), builds a records
// index, and runs every query through tbz_search_records and tbz_search_records_device with a rec_nos array of exactly
// max_hits entries on the heap (a store behind it is the sanitizer's to find).  Per query and variant it writes a line
// "status n_hits: numbers" to <out>.
#include "emu/tbz_platform.hpp"
#include "../3bz_amd/csrc/tbz_engine.hpp"

#include <fstream>
#include <iterator>
#include <sstream>

#define CHECK(call)                                                       \
  do {                                                                    \
    int r_ = (call);                                                      \
    if (r_) {                                                             \
      fprintf(stderr, "%s: %d (%s)\n", #call, r_, tbz_strerror(r_));      \
      return 1;                                                           \
    }                                                                     \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<uint8_t> z((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int format = atoi(argv[2]), delim = atoi(argv[3]);
  const size_t spacing = (size_t)atoll(argv[4]);
  tbz_ctx* ctx = nullptr;
  CHECK(tbz_ctx_create(0, &ctx));
  tbz_index* ix = nullptr;
  tbz_result res;
  CHECK(tbz_index_build_records(ctx, format, z.data(), z.size(), spacing, delim, &ix, &res));
  if (!ix || res.status != TBZ_FINISHED) return 3;
  void* d_in = nullptr;
  CHECK(tbz_device_malloc(ctx, z.size() + 64, &d_in));
  CHECK(tbz_memcpy_h2d(ctx, d_in, z.data(), z.size()));
  std::ifstream q(argv[5]);
  std::ofstream out(argv[6]);
  std::string line;
  while (std::getline(q, line)) {
    std::istringstream ls(line);
    uint64_t first, count, max_hits;
    std::string hex;
    if (!(ls >> first >> count >> max_hits >> hex)) continue;
    std::vector<uint8_t> pat;
    for (size_t i = 0; i + 1 < hex.size(); i += 2) pat.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
    for (int device = 0; device < 2; device++) {
      std::vector<uint64_t> nos(max_hits);  // exactly max_hits entries
      uint64_t n_hits = ~0ull;
      uint64_t* dst = max_hits ? nos.data() : nullptr;
      if (device)
        CHECK(tbz_search_records_device(ctx, ix, d_in, z.size(), pat.data(), pat.size(), first, count, dst, max_hits, &n_hits, &res));
      else
        CHECK(tbz_search_records(ctx, ix, z.data(), z.size(), pat.data(), pat.size(), first, count, dst, max_hits, &n_hits, &res));
      out << res.status << " " << n_hits << ":";
      for (uint64_t i = 0; i < n_hits && i < max_hits; i++) out << " " << nos[i];
      out << "\n";
    }
  }
  out.close();
  CHECK(tbz_device_free(ctx, d_in));
  tbz_index_destroy(ix);
  tbz_ctx_destroy(ctx);
  return 0;
}
