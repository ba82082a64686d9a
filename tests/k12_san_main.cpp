// TEST INFRASTRUCTURE: a stand-alone program over the engine + kernels compiled for the CPU lane emulator (as
// tests/emu/tbz_emu.cpp compiles them), built with AddressSanitizer + UBSan by tests/test_k12_san.py.
//   k12_san_main <stream> <format 0..2> <out_cap> <parts> <out>
// decodes the stream through tbz_inflate_device with a context created under TBZ_K12_PARTS=<parts>, TBZ_K12_MIN_ITEMS=1
// (the main launch, K3 and K2 in item-range parts) into an output buffer of exactly out_cap octets on the heap (a store
// behind it is the sanitizer's to find), and writes one line "status segments out_len out_total in_consumed adler32
// crc32 flags boundary_out huff_launches fnv" to <out>, fnv being FNV-1a over the out_len octets delivered.  (One decode
// per run: under the sanitizer the emulator's 64 threads per workgroup make a thousand items take a minute.)
#include "emu/tbz_platform.hpp"
#include "../3bz_amd/csrc/tbz_engine.hpp"

#include <fstream>
#include <iterator>

#define CHECK(call)                                                       \
  do {                                                                    \
    int r_ = (call);                                                      \
    if (r_) {                                                             \
      fprintf(stderr, "%s: %d (%s)\n", #call, r_, tbz_strerror(r_));      \
      return 1;                                                           \
    }                                                                     \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<uint8_t> z((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int format = atoi(argv[2]);
  const size_t cap = (size_t)atoll(argv[3]);
  std::ofstream out(argv[5]);
  setenv("TBZ_WIDE_BITS", "0", 1);  // (as tests/k12_cases.py creates its engines)
  setenv("TBZ_TOK_FULL", "1", 1);
  setenv("TBZ_K12_PARTS", argv[4], 1);
  setenv("TBZ_K12_MIN_ITEMS", "1", 1);
  tbz_ctx* ctx = nullptr;
  CHECK(tbz_ctx_create(0, &ctx));
  void *d_in = nullptr, *d_out = nullptr;
  CHECK(tbz_device_malloc(ctx, z.size() + 64, &d_in));
  CHECK(tbz_device_malloc(ctx, cap ? cap : 1, &d_out));
  CHECK(tbz_memcpy_h2d(ctx, d_in, z.data(), z.size()));
  tbz_result res;
  CHECK(tbz_inflate_device(ctx, format, d_in, z.size(), d_out, cap, &res));
  tbz_timings tim;
  CHECK(tbz_last_timings(ctx, &tim));
  if (res.out_len > cap) return 3;
  std::vector<uint8_t> got(res.out_len);
  if (res.out_len) CHECK(tbz_memcpy_d2h(ctx, got.data(), d_out, res.out_len));
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint8_t b : got) h = (h ^ b) * 0x100000001b3ull;
  out << res.status << " " << res.segments << " " << res.out_len << " " << res.out_total << " " << res.in_consumed << " "
      << res.adler32 << " " << res.crc32 << " " << res.flags << " " << res.boundary_out << " " << tim.huff_launches << " "
      << h << "\n";
  CHECK(tbz_device_free(ctx, d_in));
  CHECK(tbz_device_free(ctx, d_out));
  tbz_ctx_destroy(ctx);
  out.close();
  return 0;
}
