// TEST INFRASTRUCTURE: a stand-alone program over the engine + kernels compiled for the CPU lane emulator (as
// tests/emu/tbz_emu.cpp compiles them), built with AddressSanitizer + UBSan by tests/test_records_san.py.
//   records_san_main <stream> <format 0..2> <delim> <spacing> <runs> <out>
// reads a compressed stream and a list of runs ("first count" per line), builds a records index, exports and imports
// it, reads the runs through tbz_inflate_records (imported index) and tbz_inflate_records_device (built index), and
// writes the octets of both, run after run, to <out>.
#include "emu/tbz_platform.hpp"
#include "../3bz_amd/csrc/tbz_engine.hpp"

#include <fstream>
#include <iterator>

static std::vector<std::vector<uint8_t>*> g_bufs;
static uint8_t* alloc_octets(void*, size_t n) {
  g_bufs.push_back(new std::vector<uint8_t>(n));
  return g_bufs.back()->data();
}

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
  std::vector<uint64_t> firsts, counts;
  {
    std::ifstream r(argv[5]);
    uint64_t a, b;
    while (r >> a >> b) {
      firsts.push_back(a);
      counts.push_back(b);
    }
  }
  const size_t n = firsts.size();
  tbz_ctx* ctx = nullptr;
  CHECK(tbz_ctx_create(0, &ctx));
  tbz_index *built = nullptr, *imported = nullptr;
  tbz_result res;
  CHECK(tbz_index_build_records(ctx, format, z.data(), z.size(), spacing, delim, &built, &res));
  if (!built || res.status != TBZ_FINISHED) return 3;
  size_t need = 0;
  CHECK(tbz_index_export(built, nullptr, 0, &need));
  std::vector<uint8_t> blob(need);
  CHECK(tbz_index_export(built, blob.data(), blob.size(), &need));
  CHECK(tbz_index_import(ctx, blob.data(), blob.size(), &imported));
  int d2 = -1;
  size_t n_records = 0, n2 = 0;
  CHECK(tbz_index_records_info(built, &d2, &n_records));
  CHECK(tbz_index_records_info(imported, nullptr, &n2));
  if (d2 != delim || n2 != n_records) return 4;
  std::ofstream out(argv[6], std::ios::binary);
  // ---- the host variant, on the imported index
  std::vector<tbz_result> rr(n ? n : 1);
  CHECK(tbz_inflate_records(ctx, imported, z.data(), z.size(), n, firsts.data(), counts.data(), alloc_octets, nullptr, rr.data()));
  size_t nb = 0;
  for (size_t i = 0; i < n; i++) {
    if (rr[i].status != TBZ_FINISHED) return 5;
    if (!rr[i].out_len) continue;
    if (nb >= g_bufs.size() || g_bufs[nb]->size() != rr[i].out_len) return 6;
    out.write((const char*)g_bufs[nb]->data(), (std::streamsize)rr[i].out_len);
    nb++;
  }
  if (nb != g_bufs.size()) return 7;
  for (auto* b : g_bufs) delete b;
  // ---- the device variant, on the built index: the runs' places from a call with all capacities 0, then the octets
  void *d_in = nullptr, *d_out = nullptr;
  CHECK(tbz_device_malloc(ctx, z.size() + 64, &d_in));
  CHECK(tbz_memcpy_h2d(ctx, d_in, z.data(), z.size()));
  std::vector<uint64_t> offs(n ? n : 1, 0), caps(n ? n : 1, 0);
  CHECK(tbz_inflate_records_device(ctx, built, d_in, z.size(), n, firsts.data(), counts.data(), nullptr, offs.data(), caps.data(),
                                   rr.data()));
  uint64_t at = 3;
  for (size_t i = 0; i < n; i++) {
    if (rr[i].status != (rr[i].out_total ? TBZ_OUTPUT_OVERFLOW : TBZ_FINISHED) || rr[i].out_len) return 8;
    offs[i] = at;
    caps[i] = rr[i].out_total;
    at += caps[i] + 5;
  }
  CHECK(tbz_device_malloc(ctx, at + 64, &d_out));
  CHECK(tbz_inflate_records_device(ctx, built, d_in, z.size(), n, firsts.data(), counts.data(), d_out, offs.data(), caps.data(),
                                   rr.data()));
  std::vector<uint8_t> back(at + 64);
  CHECK(tbz_memcpy_d2h(ctx, back.data(), d_out, back.size()));
  for (size_t i = 0; i < n; i++) {
    if (rr[i].status != TBZ_FINISHED || rr[i].out_len != caps[i]) return 9;
    out.write((const char*)back.data() + offs[i], (std::streamsize)caps[i]);
  }
  out.close();
  CHECK(tbz_device_free(ctx, d_in));
  CHECK(tbz_device_free(ctx, d_out));
  tbz_index_destroy(built);
  tbz_index_destroy(imported);
  tbz_ctx_destroy(ctx);
  return 0;
}
