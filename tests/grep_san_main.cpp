// TEST INFRASTRUCTURE: a stand-alone program over the engine + kernels compiled for the CPU lane emulator (as
// tests/emu/tbz_emu.cpp compiles them), built with AddressSanitizer + UBSan by tests/test_grep_san.py.
//   grep_san_main <stream> <format 0..2> <delim> <spacing> <queries> <out>
// reads a compressed stream and a list of queries ("first count max_hits cap d_off pattern-in-hex" per line), builds a
// records index, and runs every query through tbz_grep_records and tbz_grep_records_device with, on the heap, a rec_nos
// array of exactly max_hits entries, a rec_offs array of exactly max_hits + 1 and (device variant) a destination of exactly
// cap octets behind d_off octets of guard (a store outside them is the sanitizer's to find; the guard is checked here).
// The host variant's alloc hands out exactly the octets asked for.  Per query and variant it writes a line
// "status n_hits n_out out_len out_total crc32-of-the-delivered-octets: numbers | offsets" to <out>.
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

static uint32_t crc32_of(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}

struct Handed {
  uint8_t* p = nullptr;
  size_t n = 0;
  int calls = 0;
};
static uint8_t* hand_out(void* user, size_t n) {
  Handed* h = (Handed*)user;
  h->calls++;
  h->n = n;
  h->p = (uint8_t*)malloc(n);  // exactly n octets
  return h->p;
}

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
    uint64_t first, count, max_hits, cap, d_off;
    std::string hex;
    if (!(ls >> first >> count >> max_hits >> cap >> d_off >> hex)) continue;
    std::vector<uint8_t> pat;
    for (size_t i = 0; i + 1 < hex.size(); i += 2) pat.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
    for (int device = 0; device < 2; device++) {
      uint64_t* nos = max_hits ? (uint64_t*)malloc(max_hits * 8) : nullptr;         // exactly max_hits entries
      uint64_t* offs = max_hits ? (uint64_t*)malloc((max_hits + 1) * 8) : nullptr;  // exactly max_hits + 1
      uint64_t n_hits = ~0ull, n_out = ~0ull;
      uint32_t crc = 0;
      if (device) {
        uint8_t* buf = cap ? (uint8_t*)malloc(d_off + cap) : nullptr;  // the destination ends where the allocation does
        if (buf) memset(buf, 0xA5, d_off + cap);
        CHECK(tbz_grep_records_device(ctx, ix, d_in, z.size(), pat.data(), pat.size(), first, count, buf ? buf + d_off : nullptr, cap,
                                      nos, offs, max_hits, &n_hits, &n_out, &res));
        for (uint64_t i = 0; buf && i < d_off; i++)
          if (buf[i] != 0xA5) return 4;
        for (uint64_t i = res.out_len; buf && i < cap; i++)
          if (buf[d_off + i] != 0xA5) return 5;
        if (res.out_len > cap) return 6;
        crc = crc32_of(buf ? buf + d_off : nullptr, res.out_len);
        free(buf);
      } else {
        Handed h;
        CHECK(tbz_grep_records(ctx, ix, z.data(), z.size(), pat.data(), pat.size(), first, count, hand_out, &h, cap, nos, offs,
                               max_hits, &n_hits, &n_out, &res));
        if (h.calls != (res.out_len ? 1 : 0) || (h.calls && h.n != res.out_len)) return 7;
        crc = crc32_of(h.p, h.calls ? h.n : 0);
        free(h.p);
      }
      out << res.status << " " << n_hits << " " << n_out << " " << res.out_len << " " << res.out_total << " " << crc << ":";
      const uint64_t got = n_hits < max_hits ? n_hits : max_hits;
      for (uint64_t i = 0; i < got; i++) out << " " << nos[i];
      out << " |";
      for (uint64_t i = 0; max_hits && i <= got; i++) out << " " << offs[i];
      out << "\n";
      free(nos);
      free(offs);
    }
  }
  out.close();
  CHECK(tbz_device_free(ctx, d_in));
  tbz_index_destroy(ix);
  tbz_ctx_destroy(ctx);
  return 0;
}
