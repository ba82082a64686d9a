// tbz_kernels.hpp — the device side of the inflate engine (hand-written for gfx950 / CDNA4).
//
// Every kernel runs 64-thread workgroups (one wavefront each) except the two-wave LZ77 kernel.  None of this
// is GEMM-shaped: it is integer / byte work bounded by LDS latency and instruction issue (Huffman decode,
// LZ77) or HBM bandwidth (scan, checksums), so there is no MFMA here by design.
//
//   K0  tbz_k0_scan_tiles / _offsets / _compact / _items  (+ tbz_k0_scan_emit, the second pass for crowded tiles)
//         find 00 00 FF FF flush markers (candidate independent-segment starts) in one pass of aligned
//         16-octet reads, compact them in order, build the K1 work items on the device.
//   K1h tbz_k1h_headers
//         one lane per item parses the item's first dynamic block header (code lengths) ahead of K1g.
//   K1g tbz_k1g{8,16,32,64}_huff_decode
//         a GANG of G lanes per item: gang-parallel canonical build, two-level lookup tables in the gang's
//         LDS, speculative sub-range decode with exact chain validation; tokens written once, in place,
//         as runs listed in the item's run table (replaces deflate.lisp:518-702, huffman-tree.lisp:99-218).
//   K1  tbz_k1_huff_decode
//         one LANE per item (table-free canonical decode): batches of many tiny items, and the redo of items
//         K1g declines.  Same results record, one run.
//   K2  tbz_k2_lz77_dual / tbz_k2_lz77_small / tbz_k2_lz77
//         one workgroup per group: tokens (followed through the run tables) -> LDS window -> 16-byte
//         coalesced HBM stores; matches resolved lane-parallel in rounds.  Linear window for groups that
//         fit (two waves: front end || resolve), 36 KiB ring otherwise (replaces copy-history / out-byte /
//         :copy-block, deflate.lisp:233-359,:538-573).
//   K3  tbz_k3_*
//         proof that every item landed on its successor + segment-size scan + K2's tables, on the device.
//   K4  tbz_k4_adler_partial / tbz_k4_adler_combine   (checksums.lisp:18-62)
//   K5  tbz_k5_crc_partial / tbz_k5_crc_combine       (checksums.lisp:177-210)
#pragma once
#include "tbz_platform.hpp"
#include "tbz_structs.hpp"

namespace tbz {

// ------------------------------------------------------------------------------------------------
// error / status codes used on the device (mirror include/tbz_amd.h)
// ------------------------------------------------------------------------------------------------
constexpr i32 E_BTYPE = -1, E_STORED_LEN = -2, E_OVERSUB = -3, E_INCOMPLETE = -4, E_REPEAT_NO_PREV = -5,
              E_REPEAT_OVERRUN = -6, E_INVALID_CODE = -7, E_ZLIB_HEADER = -9, E_ZLIB_DICT = -10,
              E_GZIP_MAGIC = -12, E_GZIP_METHOD = -13, E_GZIP_FLAGS = -14, E_GZIP_HCRC = -15, E_TREE_OVERFLOW = -18;

// ------------------------------------------------------------------------------------------------
// small wave helpers
// ------------------------------------------------------------------------------------------------
TBZ_DEV u32 wave_incl_scan_u32(u32 v) { return tbz_wave_incl_scan_u32(v); }
TBZ_DEV u64 wave_incl_scan_u64(u64 v) {
  const u32 lane = tbz_lane();
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    u64 t = tbz_shfl_up64(v, d);
    if (lane >= d) v += t;
  }
  return v;
}
TBZ_DEV u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += tbz_shfl_xor64(v, m);
  return v;
}
TBZ_DEV u32 wave_xor_u32(u32 v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v ^= tbz_shfl_xor(v, m);
  return v;
}

// order in which a dynamic block header lists the code-length code's lengths (constants.lisp:63-68)
TBZ_CONSTANT u8 c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// RFC 1951 length / distance bases from the symbol, in ALU (no table lookups in the hot loop).
// Same values as constants.lisp:41-61.
TBZ_DEV void len_base_extra(u32 c /* sym-257, 0..28 */, u32& base, u32& extra) {
  u32 e = (c >> 2) - 1;
  u32 b = 3 + ((4 + (c & 3)) << (e & 7));
  bool small = c < 8, top = c == 28;
  extra = (small || top) ? 0 : e;
  base = small ? 3 + c : (top ? 258 : b);
}
TBZ_DEV void dist_base_extra(u32 d /* 0..29 */, u32& base, u32& extra) {
  u32 e = (d >> 1) - 1;
  u32 b = 1 + ((2 + (d & 1)) << (e & 15));
  bool small = d < 4;
  extra = small ? 0 : e;
  base = small ? 1 + d : b;
}

// LDS accepts any octet address for 2/4/8/16-octet accesses on gfx950
struct __attribute__((packed, aligned(1))) K2U128 { u64 lo, hi; };
struct __attribute__((packed, aligned(1))) K2U64 { u64 v; };
struct __attribute__((packed, aligned(1))) K2U32 { u32 v; };
struct __attribute__((packed, aligned(1))) K2U16 { u16 v; };
TBZ_DEV u64 k2_ld64(const u8* p) { return ((const K2U64*)p)->v; }
TBZ_DEV u32 k2_ld32(const u8* p) { return ((const K2U32*)p)->v; }
TBZ_DEV void k2_st64(u8* p, u64 v) { ((K2U64*)p)->v = v; }
TBZ_DEV void k2_st32(u8* p, u32 v) { ((K2U32*)p)->v = v; }
TBZ_DEV void k2_st16(u8* p, u32 v) { ((K2U16*)p)->v = (u16)v; }

// 4 octets at byte index `idx` of a 4-byte aligned word array, never touching a word at or beyond
// `nwords` (words past the end read as 0)
TBZ_DEV u32 load_u32_unaligned(const u32* TBZ_RESTRICT w, u64 idx, u64 nwords) {
  u64 wi = idx >> 2;
  u32 sh = (u32)(idx & 3) * 8;
  u32 a = wi < nwords ? w[wi] : 0;
  if (sh == 0) return a;
  u32 b = (wi + 1) < nwords ? w[wi + 1] : 0;
  return (a >> sh) | (b << (32 - sh));
}

// ================================================================================================
// K0 — marker scan.  A marker is the BIT position of the byte AFTER `00 00 FF FF` (the LEN/NLEN of an empty stored
// block, which zlib emits for Z_SYNC_FLUSH / Z_FULL_FLUSH).  3bz has no counterpart: it is strictly
// sequential (:block-end -> :start-of-block, deflate.lisp:719-722).
// Work split: a tile is 64 KiB of MEMORY (16-octet aligned, so every load is an aligned dwordx4) =
// 64 rows of 1 KiB; lane j of row r owns the 16 octets at tile + r*1024 + j*16, a row is one fully
// coalesced 1 KiB read.  Four v_qsad_pk_u16_u8 compare the pattern against all 16 start positions
// of a lane (the three octets of lookahead come from the next lane by DPP); a packed-min tree says
// "no hit in these 16" in 10 more instructions, which is the answer for all but one row in eight.
// ================================================================================================
struct K0Params {
  const u8* in_base;
  const u64* str_off;     // per stream: byte offset / length in in_base
  const u64* str_len;
  const u32* tile_first;  // n_streams+1 prefix of tiles per stream
  u32 n_streams;
  u32 n_tiles;
  u32* tile_counts;       // [n_tiles]   markers per tile
  u32* tile_offsets;      // [n_tiles+1] (scan out; [n_tiles] = total)
  u64* markers;           // compact / emit out: in tile order, i.e. ascending within every stream
  u64* tile_slots;        // [n_tiles][K0_SLOTS]: the first markers of each tile, written by the one-pass scan
  u32* first_marker;      // [n_streams+1]: index of each stream's first marker (scan out)
  u32* head;              // [2]: total markers, tiles whose markers did not fit their slots (scan out)
  Item* items;            // item build out
  u32 format;
  u32 second_pass;        // items: the marker array was written by the emitting pass
  const u32* start_bit_off;  // per stream (nullptr: all 0): the stream's first block header sits at this bit of its first octet
                          // (resumed streams, spans entered at an index point)
  u32* n_fixed;           // items: [0] counts the marker items whose first block is a fixed-Huffman block (nullptr: not wanted) —
                          // where most are, the streams are fixed-Huffman territory and K0c looks for block chains inside them
  u32 resume;             // items: stream 0's head item carries ITEM_RESUME (a session's continuation inside a block)
};
constexpr u32 K0_SLOTS = 32;  // markers kept per 64 KiB tile by the one-pass scan (flush every 16 KiB of text: ~8)

TBZ_DEV u32 k0_find_stream(const K0Params& P, u32 tile) {
  u32 lo = 0, hi = P.n_streams;  // tile_first[lo] <= tile < tile_first[hi]
  while (hi - lo > 1) {
    u32 mid = (lo + hi) >> 1;
    if (P.tile_first[mid] <= tile) lo = mid; else hi = mid;
  }
  return lo;
}

// tiles of a stream start at its first octet's address rounded down to 16 (the host counts them the same way)
struct K0Tile {
  uintptr_t t0;          // address of the tile's first row (16-aligned)
  uintptr_t s_lo, s_hi;  // addresses of the stream's first octet and one past its last
  uintptr_t base;        // address of in_base (marker positions are relative to it)
};
TBZ_DEV K0Tile k0_tile(const K0Params& P) {
  K0Tile T;
  const u32 tile = tbz_block();
  const u32 s = k0_find_stream(P, tile);
  T.base = (uintptr_t)P.in_base;
  T.s_lo = T.base + P.str_off[s];
  T.s_hi = T.s_lo + P.str_len[s];
  T.t0 = (T.s_lo & ~(uintptr_t)15) + (uintptr_t)(tile - P.tile_first[s]) * SCAN_TILE;
  return T;
}

// 16-bit mask of marker-pattern starts among the 16 octets at address c owned by this lane:
// octet address q is a hit iff q..q+3 = 00 00 FF FF, q >= s_lo and q + 4 < s_hi
// this lane's aligned 16-octet chunk at address c (zeros outside the stream): an aligned chunk that holds at
// least one octet of the stream lies inside a mapped page
TBZ_DEV uint4 k0_load(const K0Tile& T, uintptr_t c) {
  uint4 v{};
  if (c < T.s_hi && c + 16 > T.s_lo) v = *(const uint4*)c;
  return v;
}
// `v` = k0_load(T, c) of every lane, `after` = the dword that follows lane 63's chunk
TBZ_DEV u32 k0_row_mask(const K0Tile& T, uintptr_t c, uint4 v, u32 after) {
  const u32 lane = tbz_lane();
  u32 nx = tbz_wave_shl1(v.x);
  if (lane == 63) nx = after;
  const u32 ref = 0xFFFF0000u;
  const u64 q0 = tbz_qsad4(((u64)v.y << 32) | v.x, ref), q1 = tbz_qsad4(((u64)v.z << 32) | v.y, ref);
  const u64 q2 = tbz_qsad4(((u64)v.w << 32) | v.z, ref), q3 = tbz_qsad4(((u64)nx << 32) | v.w, ref);
  u32 m0 = tbz_pk_min_u16((u32)q0, (u32)(q0 >> 32)), m1 = tbz_pk_min_u16((u32)q1, (u32)(q1 >> 32));
  u32 m2 = tbz_pk_min_u16((u32)q2, (u32)(q2 >> 32)), m3 = tbz_pk_min_u16((u32)q3, (u32)(q3 >> 32));
  m0 = tbz_pk_min_u16(tbz_pk_min_u16(m0, m1), tbz_pk_min_u16(m2, m3));
  if ((m0 & 0xffffu) != 0 && (m0 >> 16) != 0) return 0;
  u32 m = 0;
  const u64 q[4] = {q0, q1, q2, q3};
#pragma unroll
  for (u32 k = 0; k < 16; k++) {
    const uintptr_t a = c + k;
    if (((q[k >> 2] >> (16 * (k & 3))) & 0xffffu) == 0 && a >= T.s_lo && a + 4 < T.s_hi) m |= 1u << k;
  }
  return m;
}

// ONE pass over the input: count the tile's markers and keep the first K0_SLOTS of them (in order) in the
// tile's slots.  A tile with more markers than slots (stored data full of the pattern) makes the host fall
// back to the second, emitting pass below.
TBZ_KERNEL void tbz_k0_scan_tiles(K0Params P) {
  const K0Tile T = k0_tile(P);
  const u32 lane = tbz_lane();
  u64* slots = P.tile_slots + (u64)tbz_block() * K0_SLOTS;
  u32 base = 0;
  constexpr u32 ROWS = SCAN_TILE / 1024, AHEAD = 4;  // rows in flight: the loop is a chain of dependent waits otherwise
  uint4 v[AHEAD + 1];
#pragma unroll
  for (u32 q = 0; q < AHEAD; q++) v[q] = k0_load(T, T.t0 + q * 1024 + lane * 16);
  for (u32 r0 = 0; r0 < ROWS; r0 += AHEAD) {
    uint4 nv[AHEAD];
#pragma unroll
    for (u32 q = 0; q < AHEAD; q++)  // (past the tile only the row whose first dword follows the tile's last chunk)
      nv[q] = (r0 + AHEAD + q < ROWS || q == 0) ? k0_load(T, T.t0 + (r0 + AHEAD + q) * 1024 + lane * 16) : uint4{};
    v[AHEAD] = nv[0];
#pragma unroll
    for (u32 q = 0; q < AHEAD; q++) {
      const uintptr_t c = T.t0 + (r0 + q) * 1024 + lane * 16;
      u32 m = k0_row_mask(T, c, v[q], tbz_readlane(v[q + 1].x, 0));  // the next row's first dword follows lane 63
      if (tbz_ballot(m != 0) != 0) {                                 // wave-uniform: something in this row
        u32 n = __builtin_popcount(m);
        u32 inc = wave_incl_scan_u32(n);
        u32 o = base + inc - n;
        while (m) {
          u32 k = __builtin_ctz(m);
          m &= m - 1;
          if (o < K0_SLOTS) slots[o] = ((u64)(c + k - T.base) + 4) * 8;
          o++;
        }
        base += tbz_shfl(inc, 63);
      }
    }
#pragma unroll
    for (u32 q = 0; q < AHEAD; q++) v[q] = nv[q];
  }
  if (lane == 0) P.tile_counts[tbz_block()] = base;
}

// single-wave exclusive scan over tile counts
// (ONE workgroup of 1024 threads, 1024 tiles per step: a single wave took 30 us for config 2's 16 384 tiles)
constexpr u32 K0_SCAN_THREADS = 1024;
TBZ_KERNEL_WG(1024, 1) void tbz_k0_scan_offsets(K0Params P) {
  TBZ_SHARED u32 wsum[16];
  TBZ_SHARED u32 wover[16];
  const u32 lane = tbz_lane(), wave = tbz_wave(), tid = wave * 64 + lane;
  u32 carry = 0, over = 0;
  for (u32 i = 0; i < P.n_tiles; i += K0_SCAN_THREADS) {  // uniform over the workgroup
    const bool in = i + tid < P.n_tiles;
    const u32 v = in ? P.tile_counts[i + tid] : 0;
    over += v > K0_SLOTS ? 1u : 0u;
    const u32 inc = wave_incl_scan_u32(v);
    if (lane == 63) wsum[wave] = inc;
    tbz_wg_barrier();
    u32 before = 0, total = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
      const u32 x = wsum[k];
      before += k < wave ? x : 0u;
      total += x;
    }
    if (in) P.tile_offsets[i + tid] = carry + before + inc - v;
    carry += total;
    tbz_wg_barrier();  // wsum is rewritten in the next step
  }
  over = (u32)wave_sum_u64(over);
  if (lane == 0) wover[wave] = over;
  tbz_wg_barrier();
  if (tid == 0) {
    u32 ov = 0;
    for (u32 k = 0; k < 16; k++) ov += wover[k];
    if (P.n_fixed) P.n_fixed[0] = P.n_fixed[1] = 0;  // (tbz_k0_items, launched after this kernel, counts into them)
    P.tile_offsets[P.n_tiles] = carry;
    P.head[0] = carry;
    P.head[1] = ov;
  }
}

// slots -> the compact marker array; markers come out in tile order, so a stream's markers are the ones of
// its tiles (workgroup 0 writes the per-stream index)
TBZ_KERNEL void tbz_k0_compact(K0Params P) {
  const u32 lane = tbz_lane(), t = tbz_block();
  const u32 n = P.tile_counts[t], o = P.tile_offsets[t];
  // crowded tiles (head[1]): the marker array is sized for the slots only; the host runs the emitting pass
  if (P.head[1] == 0 && lane < n) P.markers[o + lane] = P.tile_slots[(u64)t * K0_SLOTS + lane];
  if (t == 0)
    for (u32 s = lane; s <= P.n_streams; s += 64) P.first_marker[s] = P.tile_offsets[s < P.n_streams ? P.tile_first[s] : P.n_tiles];
}

// items: per stream one head item (the stream's first octet) and one per marker
TBZ_KERNEL void tbz_k0_items(K0Params P) {
  const u32 i = tbz_block() * 64 + tbz_lane();
  const u32 n_items = P.head[0] + P.n_streams;
  if (i >= n_items || (P.head[1] != 0 && !P.second_pass)) return;  // crowded tiles: wait for the emitting pass
  u32 lo = 0, hi = P.n_streams;  // first_item[s] = first_marker[s] + s; find s with first_item[s] <= i < first_item[s+1]
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (P.first_marker[mid] + mid <= i) lo = mid; else hi = mid;
  }
  const u32 s = lo, fm = P.first_marker[s], nm = P.first_marker[s + 1] - fm;
  const u32 k = i - (fm + s);
  Item it;
  it.start_bit = k == 0 ? P.str_off[s] * 8 + (P.start_bit_off ? P.start_bit_off[s] : 0u) : P.markers[fm + k - 1];
  it.limit_bit = k < nm ? P.markers[fm + k] : ~0ull;
  it.end_byte = P.str_off[s] + P.str_len[s];
  it.stream = s;
  it.flags = (P.format << ITEM_FMT_SHIFT) | (k == 0 ? ITEM_HEAD : 0u) | ((i == 0 && P.resume) ? ITEM_RESUME : 0u);
  P.items[i] = it;
  if (P.n_fixed) {  // BTYPE of the block at a marker (markers are octet positions; the stream has at least one octet there)
    bool fx = false;
    if (k != 0 && (it.start_bit >> 3) < it.end_byte) fx = ((P.in_base[it.start_bit >> 3] >> 1) & 3) == 1;
    if (fx) tbz_atomic_add_global(P.n_fixed, 1u);  // (lanes past the list have left: no collective here)
    // n_fixed[1]: the streams that BEGIN with a stored block (raw deflate and zlib: the first block header sits at a known
    // place) — such a stream is stored data more likely than not, and a search for Huffman block headers in it is wasted
    if (k == 0 && P.format != 2) {
      const u64 hb = it.start_bit + (P.format == 1 ? 16u : 0u);
      if ((hb >> 3) + 1 < it.end_byte) {
        const u32 v = ((u32)P.in_base[hb >> 3] | ((u32)P.in_base[(hb >> 3) + 1] << 8)) >> (hb & 7);
        if (((v >> 1) & 3) == 0) tbz_atomic_add_global(P.n_fixed + 1, 1u);
      }
    }
  }
}

TBZ_KERNEL void tbz_k0_scan_emit(K0Params P) {
  const K0Tile T = k0_tile(P);
  const u32 lane = tbz_lane();
  u32 base = P.tile_offsets[tbz_block()];
  for (u32 r = 0; r < SCAN_TILE / 1024; r++) {
    const uintptr_t c = T.t0 + r * 1024 + lane * 16;
    const uintptr_t ca = T.t0 + r * 1024 + 1024;  // the dword after lane 63's chunk
    u32 m = k0_row_mask(T, c, k0_load(T, c), (ca < T.s_hi && ca + 16 > T.s_lo) ? *(const u32*)ca : 0u);
    if (tbz_ballot(m != 0) == 0) continue;  // wave-uniform: nothing in this row
    u32 n = __builtin_popcount(m);
    u32 inc = wave_incl_scan_u32(n);
    u32 o = base + inc - n;
    while (m) {
      u32 k = __builtin_ctz(m);
      m &= m - 1;
      P.markers[o++] = ((u64)(c + k - T.base) + 4) * 8;
    }
    base += tbz_shfl(inc, 63);
  }
}

// ================================================================================================
// K0g — gzip member starts.  A .gz file may hold many members back to back (RFC 1952 2.2); 3bz decodes the first and
// stops (gzip.lisp:277-286), leaving the caller to call again at the next member — whose start is only known once
// the member before it has been decoded.  Same move as for flush markers: every `1f 8b 08` with a legal FLG octet
// (gzip.lisp:113-139) is a CANDIDATE start, all candidate ranges are decoded as one batch, and a candidate is a
// member iff its predecessor FINISHED exactly there (tbz_inflate_gzip_members_device).  A record also carries the four
// octets before the candidate: the ISIZE of the member that ends there, if one does — the size of its output buffer
// (unchecked by the reference, gzip.lisp:96-101; a wrong one shows as output-overflow and the member is decoded again).
// Records are appended in no particular order (one atomic per wave that found any); the host sorts them.
// ================================================================================================
struct GzCand {
  u64 pos;     // octet offset of the `1f`
  u32 before;  // the little-endian u32 that ends at pos (0 for pos < 4)
  u32 pad;
};
struct K0gParams {
  const u8* in;
  u64 in_len;
  GzCand* cands;
  u32* count;   // [0] candidates found (may exceed cap: the host grows the list and scans again)
  u32 cap;
};
TBZ_KERNEL void tbz_k0g_scan(K0gParams P) {
  const u32 lane = tbz_lane();
  const uintptr_t a0 = (uintptr_t)P.in & ~(uintptr_t)15;                 // 16-octet aligned rows of 1 KiB
  const uintptr_t lo = (uintptr_t)P.in, hi = lo + P.in_len;
  const uintptr_t c = a0 + (uintptr_t)tbz_block() * 1024 + lane * 16;    // this lane's chunk
  uint4 v{};
  if (c < hi && c + 16 > lo) v = *(const uint4*)c;                       // (an aligned chunk holding a stream octet is mapped)
  u32 nx = tbz_wave_shl1(v.x);
  if (lane == 63) {
    const uintptr_t cn = c + 16;
    nx = (cn < hi && cn + 16 > lo) ? *(const u32*)cn : 0u;
  }
  const u32 w[5] = {v.x, v.y, v.z, v.w, nx};
  u32 m = 0;
#pragma unroll
  for (u32 k = 0; k < 16; k++) {
    const u32 x = tbz_alignbit(w[(k >> 2) + 1], w[k >> 2], 8 * (k & 3));  // the four octets at chunk offset k
    const uintptr_t a = c + k;
    if ((x & 0xffffffu) == 0x088b1fu && (x >> 29) == 0 && a >= lo && a + 4 <= hi) m |= 1u << k;
  }
  const u64 any = tbz_ballot(m != 0);
  if (any == 0) return;  // wave-uniform
  const u32 n = (u32)__builtin_popcount(m);
  const u32 inc = tbz_wave_incl_scan_u32(n);
  u32 base = 0;
  if (lane == 63) base = tbz_atomic_add_global(P.count, inc);
  base = tbz_shfl(base, 63);
  u32 at = base + inc - n;
  while (m) {
    const u32 k = (u32)__builtin_ctz(m);
    m &= m - 1;
    if (at < P.cap) {
      GzCand g;
      g.pos = (u64)(c + k - lo);
      g.before = 0;
      if (g.pos >= 4) {
        const u8* q = P.in + g.pos - 4;
        g.before = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24);
      }
      g.pad = 0;
      P.cands[at] = g;
    }
    at++;
  }
}

// ================================================================================================
// K0b — block-start finder for streams WITHOUT flush markers.  DEFLATE blocks are bit-aligned
// and unmarked: 3bz finds the next block only by finishing the previous one (:block-end -> :start-of-block,
// deflate.lisp:719-722).  But the header of a dynamic-Huffman block (deflate.lisp:577-669) is heavily
// redundant, so plausible headers can be FOUND: every bit position is tested for
//     BFINAL=0 (1 near the stream's end), BTYPE=2 | HLIT <= 29, HDIST <= 29 | the code-length code is complete (Kraft sum exactly 1)
// by tbz_k0b_scan (bit-parallel masks over 32 positions at a time, then one LDS lookup per four code
// lengths: ~1 position in 2300 survives on compressed data), and the survivors are parsed in full by
// tbz_k0b_validate, one lane each: the HLIT+HDIST code lengths must decode without a repeat error, the
// literal/length code must be complete and hold the end-of-block symbol, the distance code complete or a
// single symbol (what is left is a true block start, or a false positive every few hundred MB).
// A candidate is only ever USED if the block chain lands on it exactly (tbz_engine.hpp): a false candidate
// costs a repair launch, never a wrong octet; a missed true start costs parallelism, nothing else.
// Fixed-Huffman and stored blocks carry no such redundancy and are not looked for: the item before them
// decodes through them.
// ================================================================================================
#ifdef TBZ_WAVE_TRACE
#define TBZ_TR_NOW() wall_clock64()
#else
#define TBZ_TR_NOW() 0ull
#endif
#ifdef TBZ_WAVE_TRACE
__device__ u32 tbz_exp_flags;  // experiment builds (tools/exp): switches parts of kernels off to see what they cost
__device__ u64 tbz_dbg[8192 * 8];
__device__ u32 tbz_dbg_cnt[4];
#endif
constexpr u32 K0B_TILE = 8u << 10;   // octets of memory per finder workgroup (8 rows of 1 KiB)
constexpr u32 K0B_SLOTS = 128;       // survivors kept per tile (expected ~28 on compressed data, twice that near a stream's end,
                                     // where BFINAL = 1 passes too; more are dropped): ONE pass of tbz_k0b_validate nearly always
constexpr u32 K0B_TAIL_BITS = 80;    // a candidate must have this much stream left (3+14+up to 57 header bits)
constexpr u32 K0B_PRE_WORDS = 32;    // words of a candidate's header staged in LDS up front (128 octets)
constexpr u32 K0B_FINAL_WINDOW = 128u << 10;  // octets before a stream's end in which a header with BFINAL = 1 is a candidate
struct K0bParams {
  const u8* in_base;
  const u64* str_off;
  const u64* str_len;
  const u32* tile_first;   // [n_streams+1] prefix of FINDER tiles per stream (a stream that is not searched has none)
  u32 n_streams;
  u32 n_tiles;
  u64* slots;              // [n_tiles][K0B_SLOTS] candidate bit positions (relative to in_base), ascending
  u32* counts;             // [n_tiles]
  u32* offsets;            // [n_tiles+1] exclusive scan of counts
  u64* cands;              // compacted candidates (stream order, ascending)
  u32* first_cand;         // [n_streams+1]
  u32* head;               // [1]: total candidates
  const u64* markers;      // merge: K0's flush markers (bit positions) ...
  const u32* first_marker; //   [n_streams+1]
  u64* merged;             // ... and the merged list
  u32* first_merged;       //   [n_streams+1]
  u32* head_merged;        //   [2]: total, 0  (laid out as K0Params::head for tbz_k0_items)
  const u32* start_bit_off;  // per stream (nullptr: all 0): the stream begins at this bit of its first octet: nothing before it
                           // is a candidate
  u32 slots_per_tile;      // K0B_SLOTS for the dynamic-header finder, K0C_SLOTS for the fixed-chain finder
  u32 pair;                // tbz_k0b_validate: 1 = two tiles per wave (32 lanes each), for launches of many waves
  u64* ends;               // K0c: [n_tiles][slots_per_tile] where the block that starts at the slot's candidate ends (0: nowhere)
  u8* link;                // K0c: [n_tiles][slots_per_tile][2]: [0] some candidate's block ends here, [1] ... and on THAT
                           //   candidate a block ends too
  u64* keep;               // [n_tiles][slots_per_tile / 64]: which of a tile's `counts` slots survive the spacing rule
  u32* kcounts;            // [n_tiles]: how many (what tbz_k0b_offsets scans)
  u64 max_block;           // K0c: bits after which a skimmed block is given up (K0C_MAX_BLOCK)
};
TBZ_DEV u32 k0b_find_stream(const K0bParams& P, u32 tile) {
  u32 lo = 0, hi = P.n_streams;  // tile_first[lo] <= tile < tile_first[hi]; streams without tiles are skipped over
  while (hi - lo > 1) {
    u32 mid = (lo + hi) >> 1;
    if (P.tile_first[mid] <= tile) lo = mid; else hi = mid;
  }
  return lo;
}
TBZ_DEV u32 k0b_kraft3(u32 l) { return (128u >> l) & 0x7fu; }  // 2^(7-l), 0 for an unused symbol

TBZ_KERNEL void tbz_k0b_scan(K0bParams P) {
  TBZ_SHARED u16 T[4096];  // Kraft sum (units of 2^-7) of four 3-bit code lengths
  const u32 lane = tbz_lane();
  for (u32 i = lane; i < 4096; i += 64)
    T[i] = (u16)(k0b_kraft3(i & 7) + k0b_kraft3((i >> 3) & 7) + k0b_kraft3((i >> 6) & 7) + k0b_kraft3((i >> 9) & 7));
  tbz_sync();
  const u32 tile = tbz_block();
  const u32 s = k0b_find_stream(P, tile);
  const uintptr_t base = (uintptr_t)P.in_base;
  const uintptr_t s_lo = base + P.str_off[s], s_hi = s_lo + P.str_len[s];
  const uintptr_t t0 = (s_lo & ~(uintptr_t)15) + (uintptr_t)(tile - P.tile_first[s]) * K0B_TILE;
  // candidate bit positions p (relative to in_base) must satisfy p_min <= p <= p_max
  const u64 p_min = (u64)(s_lo - base) * 8 + 1 + (P.start_bit_off ? P.start_bit_off[s] : 0u);  // (the stream's first bit belongs to the head item)
  const u64 p_end = (u64)(s_hi - base) * 8;
  u64* slots = P.slots + (u64)tile * P.slots_per_tile;
  u32 nout = 0;
  // BFINAL = 1 is accepted near the stream's end only (the final block starts within one block's length of it; everywhere
  // else the extra bit halves the survivors)
  const u64 final_ok = t0 + K0B_FINAL_WINDOW >= s_hi ? ~0ull : 0ull;
  for (u32 r = 0; r < K0B_TILE / 1024; r++) {
    const uintptr_t c = t0 + r * 1024 + lane * 16;
    if (t0 + r * 1024 >= s_hi) break;  // wave-uniform: the rest of the tile lies past the stream
    u32 w[7];
    uint4 v{};
    if (c < s_hi && c + 16 > s_lo) v = *(const uint4*)c;  // an aligned chunk holding a stream octet is mapped
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    w[4] = tbz_wave_shl1(v.x);
    w[5] = tbz_wave_shl1(v.y);
    w[6] = tbz_wave_shl1(v.z);
    if (lane == 63) {
      uint4 nx{};
      const uintptr_t cn = c + 16;
      if (cn < s_hi && cn + 16 > s_lo) nx = *(const uint4*)cn;
      w[4] = nx.x; w[5] = nx.y; w[6] = nx.z;
    }
    const u64 bit0 = (u64)(c - base) * 8;  // may wrap below in_base for the first chunk: those positions fail p_min
    u32 found = 0, nf = 0;                 // up to four survivors per lane: their offsets 0..127, one octet each
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
      const u64 x = ((u64)w[k + 1] << 32) | w[k];
      const u64 m = (~x | final_ok) & ~(x >> 1) & (x >> 2);                  // BFINAL 0, BTYPE 2 (bits 0,0,1)
      const u64 hl = (x >> 4) & (x >> 5) & (x >> 6) & (x >> 7);              // HLIT >= 30
      const u64 hd = (x >> 9) & (x >> 10) & (x >> 11) & (x >> 12);           // HDIST >= 30
      u32 m32 = (u32)(m & ~hl & ~hd);
      while (m32) {
        const u32 o = (u32)__builtin_ctz(m32);
        m32 &= m32 - 1;
        const u64 p = bit0 + 32 * k + o;
        // HCLEN and the code-length code's lengths: 61 bits from o+13 on (x holds 51 - o of them, the next word 32)
        u64 f = (x >> (o + 13)) | ((u64)w[k + 2] << (51 - o));
        if (o > 19) f |= (u64)w[k + 3] << (83 - o);
        const u32 n = (u32)(f & 15) + 4;
        u64 L = f >> 4;
        L &= (1ull << (3 * n)) - 1;  // 3n <= 57
        const u32 sum = (u32)T[L & 4095] + T[(L >> 12) & 4095] + T[(L >> 24) & 4095] + T[(L >> 36) & 4095] +
                        T[(L >> 48) & 4095];
        const bool ok = sum == 128 && (i64)p >= (i64)p_min && p + K0B_TAIL_BITS <= p_end && (i64)p > 0;
        if (ok && nf < 4) {
          found |= (32 * k + o) << (8 * nf);
          nf++;
        }
      }
    }
    if (tbz_ballot(nf != 0) == 0) continue;  // wave-uniform
    const u32 inc = wave_incl_scan_u32(nf);
    u32 at = nout + inc - nf;
    for (u32 j = 0; j < nf; j++, at++)
      if (at < K0B_SLOTS) slots[at] = bit0 + ((found >> (8 * j)) & 0xffu);
    nout += tbz_shfl(inc, 63);
  }
  if (lane == 0) P.counts[tile] = nout < K0B_SLOTS ? nout : K0B_SLOTS;
}

// ---- full parse of one surviving candidate (one lane): a lean restatement of :dynamic-huffman-block …
// :dht-len-table-data (deflate.lisp:577-669) that keeps no code lengths, only their Kraft sums
struct K0bBits {
  const u32* w;   // word base, 16-octet aligned
  u64 wi;         // next word to hand out
  u64 nwords;
  u64 buf;        // LSB-first bit buffer
  u32 n;          // valid bits in buf
  uint4 q;        // the aligned four words that hold word wi (fetched 16 octets at a time: a header is a serial
  u64 qi;         //   read of 60-150 octets, and every fetch is a memory round trip for the whole wave)
  const u32* pre; // LDS [K0B_PRE_WORDS][64]: the candidate's first octets, loaded in one go (nullptr: none).  The lanes of
  u64 pre0;       //   a wave are out of step, so on-demand fetches put one memory round trip into nearly EVERY trip of
                  //   the symbol loop (measured: 346 us for 110 000 candidates, most of them rejected within 40 octets)
};
TBZ_DEV u32 k0b_word(K0bBits& b) {
  const u64 i = b.wi++;
  if (b.pre && i - b.pre0 < K0B_PRE_WORDS) return b.pre[(i - b.pre0) * 64 + tbz_lane()];  // (already masked at the stream's end)
  if ((i & ~3ull) != b.qi) {
    b.qi = i & ~3ull;
    b.q = b.qi < b.nwords ? *(const uint4*)(b.w + b.qi) : uint4{};  // (an aligned 16-octet chunk that holds a stream octet is mapped)
  }
  const u32 k = (u32)(i & 3);
  const u32 v = k == 0 ? b.q.x : k == 1 ? b.q.y : k == 2 ? b.q.z : b.q.w;
  return i < b.nwords ? v : 0u;
}
TBZ_DEV void k0b_need(K0bBits& b, u32 k) {  // k <= 32
  while (b.n < k) {
    b.buf |= (u64)k0b_word(b) << b.n;
    b.n += 32;
  }
}
TBZ_DEV u32 k0b_take(K0bBits& b, u32 k) {  // k <= 16
  k0b_need(b, k);
  const u32 v = (u32)b.buf & ((1u << k) - 1);
  b.buf >>= k;
  b.n -= k;
  return v;
}
TBZ_DEV bool k0b_validate_one(const u8* in_base, u64 p, u64 s_lo_bit, u64 p_end, u32* pre) {
  const u32 lane = tbz_lane();
  // the block that follows a flush marker is K0's: no duplicates
  if ((p & 7) == 0 && p >= s_lo_bit + 32) {
    const u8* q = in_base + (p >> 3) - 4;
    if (q[0] == 0 && q[1] == 0 && q[2] == 0xff && q[3] == 0xff) return false;
  }
  K0bBits b;
  const uintptr_t a0 = (uintptr_t)in_base;
  const u32 mis = (u32)(a0 & 15);
  b.w = (const u32*)(a0 - mis);
  const u64 a = p + mis * 8;
  b.nwords = (mis * 8 + p_end + 31) >> 5;
  b.wi = a >> 5;
  b.qi = ~0ull;
  b.q = uint4{};
  b.buf = 0;
  b.n = 0;
  b.pre = pre;
  b.pre0 = b.wi & ~3ull;
  if (pre) {  // eight independent 16-octet loads: one round trip
#pragma unroll
    for (u32 k = 0; k < K0B_PRE_WORDS; k += 4) {
      const u64 wq = b.pre0 + k;
      const uint4 v = wq < b.nwords ? *(const uint4*)(b.w + wq) : uint4{};
      pre[(k + 0) * 64 + lane] = wq + 0 < b.nwords ? v.x : 0u;
      pre[(k + 1) * 64 + lane] = wq + 1 < b.nwords ? v.y : 0u;
      pre[(k + 2) * 64 + lane] = wq + 2 < b.nwords ? v.z : 0u;
      pre[(k + 3) * 64 + lane] = wq + 3 < b.nwords ? v.w : 0u;
    }
  }
#ifdef TBZ_WAVE_TRACE
  if (tbz_exp_flags & 4) return false;
#endif
  k0b_need(b, 32);
  b.buf >>= (a & 31);
  b.n -= (u32)(a & 31);
  u64 used = 3 + 14;
  k0b_take(b, 3);
  const u32 hlit = k0b_take(b, 5) + 257, hdist = k0b_take(b, 5) + 1, hclen = k0b_take(b, 4) + 4;
  // code-length code: lengths by symbol, 3 bits each
  u64 pl = 0;
  u32 cnt = 0;  // eight 4-bit counters: codes per length 0..7 (a length used 16+ times cannot be complete: 19 symbols)
  for (u32 i = 0; i < hclen; i++) {
    const u32 l = k0b_take(b, 3);
    pl |= (u64)l << (3 * c_cl_order[i]);
    if (l) cnt += 1u << (4 * l);
  }
  used += 3 * hclen;
  // The code-length code is decoded out of REGISTERS (canonical compare-count; no table: building a 128-entry table
  // per lane cost 70 us of LDS stores per pass, and every lookup was an LDS round trip in a serial chain):
  //   lim[l]  (8 bits each)  left-aligned 7-bit limit of the codes of length <= l
  //   dlt[l]  (8 bits each)  canonical slot of a code c of length l = (c + dlt[l]) & 31
  //   sorted  (5 bits each)  symbols in canonical order: by length, then by symbol
  u64 limv = 0, dltv = 0, s0 = 0, s1 = 0;
  {
    u32 code = 0, prev = 0, off = 0;
    u64 posv = 0;  // first slot of each length, 5 bits each
    for (u32 l = 1; l < 8; l++) {
      code = (code + prev) << 1;
      prev = (cnt >> (4 * l)) & 15;
      limv |= (u64)(((code + prev) << (7 - l)) & 0xffu) << (8 * l);  // 128 (a complete code's last limit) is stored as 0x80
      dltv |= (u64)((off - code) & 0xffu) << (8 * l);
      posv |= (u64)off << (5 * l);
      off += prev;
    }
    for (u32 sym = 0; sym < 19; sym++) {
      const u32 l = (u32)(pl >> (3 * sym)) & 7;
      if (!l) continue;
      const u32 at = (u32)(posv >> (5 * l)) & 31;
      posv += 1ull << (5 * l);
      if (at < 12) s0 |= (u64)sym << (5 * at);
      else s1 |= (u64)sym << (5 * (at - 12));
    }
  }
#ifdef TBZ_WAVE_TRACE
  if (tbz_exp_flags & 8) return false;
#endif
  const u32 n = hlit + hdist;
  u32 i = 0, last = 0xff, kl = 0, kd = 0, nl_used = 0, nd_used = 0;
  bool eob = false;
  while (i < n) {
#ifdef TBZ_WAVE_TRACE
    if (lane == (u32)__builtin_ctzll(tbz_ballot(true))) atomicAdd(&pre[K0B_PRE_WORDS * 64], 1u);
#endif
    k0b_need(b, 16);
    const u32 r7 = tbz_brev32((u32)b.buf) >> 25;
    u32 l = 1;
#pragma unroll
    for (u32 k = 1; k < 7; k++) l += r7 >= ((u32)(limv >> (8 * k)) & 0xffu) ? 1u : 0u;
    if (l == 7 && r7 >= ((u32)(limv >> 56) & 0xffu) && ((u32)(limv >> 56) & 0xffu) != 0x80u) return false;  // (not reached: the scan kept complete codes only)
    const u32 slot = ((r7 >> (7 - l)) + ((u32)(dltv >> (8 * l)) & 0xffu)) & 31;
    const u32 sym = slot < 12 ? (u32)(s0 >> (5 * slot)) & 31 : (u32)(s1 >> (5 * (slot - 12))) & 31;
    const u32 xb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
    const u32 x = ((u32)(b.buf >> l)) & ((1u << xb) - 1);
    b.buf >>= l + xb;
    b.n -= l + xb;
    used += l + xb;
    u32 rep = 1, val = sym;
    if (sym == 16) {
      if (last >= 16) return false;
      rep = 3 + x;
      val = last;
    } else if (sym == 17) {
      rep = 3 + x;
      val = 0;
    } else if (sym == 18) {
      rep = 11 + x;
      val = 0;
    }
    if (i + rep > n) return false;
    last = val;
    if (val) {
      const u32 nlit = i < hlit ? (hlit - i < rep ? hlit - i : rep) : 0u;
      const u32 kr = 32768u >> val;
      kl += nlit * kr;
      kd += (rep - nlit) * kr;
      nl_used += nlit;
      nd_used += rep - nlit;
      if (i <= 256 && 256 < i + rep) eob = true;
      if (kl > 32768u || kd > 32768u) return false;  // over-subscribed (huffman-tree.lisp:116-117)
    }
    i += rep;
  }
  if (p + used > p_end) return false;
  if (!eob || kl != 32768u) return false;                 // literal/length code: complete, with end-of-block
  if (kd != 32768u && nd_used > 1) return false;          // distance code: complete, or at most one symbol
  return true;
}

// One wave serves TWO tiles, 32 lanes each: a tile holds ~28 survivors, and nearly every tile holds one that parses for
// 150+ symbols (a true header, or a false one whose lengths stay far below a complete code), so a wave per tile ran a
// median of 165 trips of the symbol loop with 28 of 64 lanes occupied at the start.
TBZ_KERNEL void tbz_k0b_validate(K0bParams P) {
#ifdef TBZ_WAVE_TRACE
  TBZ_SHARED u32 pre[K0B_PRE_WORDS * 64 + 4];
  const u64 tr0 = wall_clock64();
  if (tbz_lane() == 0) pre[K0B_PRE_WORDS * 64] = 0;
  tbz_sync();
#else
  TBZ_SHARED u32 pre[K0B_PRE_WORDS * 64];  // per lane: the first 128 octets of its candidate
#endif
  // (P.pair = 0: one tile per wave — fewer trips per wave, better where the launch fits the chip at once)
  const u32 lane = tbz_lane(), half = P.pair ? lane >> 5 : 0u, hl = P.pair ? lane & 31 : lane, W = P.pair ? 32u : 64u;
  const u32 tile = P.pair ? 2 * tbz_block() + half : tbz_block();
  const bool have = tile < P.n_tiles;
  const u32 s = have ? k0b_find_stream(P, tile) : 0;
  const u64 s_lo_bit = P.str_off[s] * 8, p_end = (P.str_off[s] + P.str_len[s]) * 8;
  u64* slots = P.slots + (u64)(have ? tile : 0) * P.slots_per_tile;
  const u32 count = have ? P.counts[tile] : 0;
  const u32 c0 = tbz_shfl(count, 0), c1 = tbz_shfl(count, 32);
  const u32 cmax = c0 > c1 ? c0 : c1;
  u32 nout = 0;
  for (u32 j0 = 0; j0 < cmax; j0 += W) {  // wave-uniform trip count
    const u32 j = j0 + hl;
    u64 p = 0;
    bool ok = false;
    if (j < count) {
      p = slots[j];
      ok = k0b_validate_one(P.in_base, p, s_lo_bit, p_end, pre);
    }
    u64 okm = tbz_ballot(ok);
    if (P.pair) okm = (okm >> (32 * half)) & 0xffffffffull;  // my tile's half of the wave
    tbz_sync();  // every lane has read its slot before the compacted ones are written (out index <= j)
    if (ok) slots[nout + tbz_popc64(okm & ((1ull << hl) - 1))] = p;
    nout += tbz_popc64(okm);
    tbz_sync();
  }
  if (hl == 0 && have) P.counts[tile] = nout;
#ifdef TBZ_WAVE_TRACE
  tbz_sync();
  if (lane == 0 && tile < 8192) {
    tbz_dbg[tile * 8 + 0] = tr0;
    tbz_dbg[tile * 8 + 1] = wall_clock64();
    tbz_dbg[tile * 8 + 2] = pre[K0B_PRE_WORDS * 64];
    tbz_dbg[tile * 8 + 3] = count;
    tbz_dbg[tile * 8 + 4] = nout;
  }
#endif
}

// Items must start at least 2^RUN_SHIFT bits apart: an item's run table is addressed by its start position (one slot per
// 2^RUN_SHIFT bits, and every item owns at least one slot), so two starts inside one slot's span would share it.  Flush
// markers keep that distance among themselves (a marker is five octets); candidates do not — a Z_BLOCK-flushed fixed
// block of one or two literals is 17-28 bits long, and the dynamic block after it is a candidate right behind a
// marker, the stream's head or another candidate.  Rule (K0C_SPACING bits, for K0b's and K0c's candidates alike): a
// candidate is dropped when a marker or the stream's head lies within the spacing on either side, or another candidate
// of the (immutable) list before it does — dropped or not, so the decision needs no order among workgroups.  The item
// before a dropped candidate simply decodes through it.  The verdict is a bit mask per tile; tbz_k0b_compact applies it.
constexpr u64 K0C_SPACING = 128;
static_assert(K0C_SPACING >= (1ull << RUN_SHIFT), "item starts must not share a run-table slot");
TBZ_DEV bool k0x_marker_near(const K0bParams& P, u32 s, u64 p) {
  u32 lo = P.first_marker[s];
  const u32 m_hi = P.first_marker[s + 1];
  u32 hi = m_hi;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (P.markers[mid] + K0C_SPACING <= p) lo = mid + 1; else hi = mid;
  }
  return lo < m_hi && P.markers[lo] < p + K0C_SPACING;
}
// the last slot of the tile before (same stream), or 0: whatever lies further back is a tile away
TBZ_DEV u64 k0x_prev_tile_last(const K0bParams& P, u32 s, u32 tile) {
  if (tile <= P.tile_first[s]) return 0;
  const u32 cp = P.counts[tile - 1];
  return cp ? P.slots[(u64)(tile - 1) * P.slots_per_tile + cp - 1] : 0;
}
// `ok`: the lane's slot j0 + lane passes every other test; `p` its position.  Returns the keep verdict: ok, no
// marker / head near, no slot of the list within the spacing before it (`carry`: the last slot before this chunk).
TBZ_DEV bool k0x_spaced(const K0bParams& P, u32 s, u64 head, u64 p, bool have, bool ok, u64& carry) {
  const u32 lane = tbz_lane();
  if (ok) ok = p >= head + K0C_SPACING && !k0x_marker_near(P, s, p);
  const u32 b_lo = tbz_wave_shr1((u32)p), b_hi = tbz_wave_shr1((u32)(p >> 32));
  const u64 before = lane == 0 ? carry : (((u64)b_hi << 32) | b_lo);
  const u64 hm = tbz_ballot(have);
  if (hm) carry = tbz_shfl64(p, 63 - (int)__builtin_clzll(hm));
  return ok && (before == 0 || p - before >= K0C_SPACING);
}
TBZ_KERNEL void tbz_k0b_space(K0bParams P) {
  const u32 lane = tbz_lane(), tile = tbz_block();
  const u32 s = k0b_find_stream(P, tile);
  const u64* slots = P.slots + (u64)tile * P.slots_per_tile;
  const u32 count = P.counts[tile];
  const u64 head = P.str_off[s] * 8 + (P.start_bit_off ? P.start_bit_off[s] : 0u);
  u64 carry = k0x_prev_tile_last(P, s, tile);
  u32 kept = 0;
  for (u32 j0 = 0; j0 < P.slots_per_tile; j0 += 64) {  // wave-uniform trip count; every mask word is written
    const bool have = j0 + lane < count;
    const u64 p = have ? slots[j0 + lane] : 0;
    const u64 km = tbz_ballot(k0x_spaced(P, s, head, p, have, have, carry));
    if (lane == 0) P.keep[(u64)tile * (P.slots_per_tile / 64) + j0 / 64] = km;
    kept += tbz_popc64(km);
  }
  if (lane == 0) P.kcounts[tile] = kept;
}

// ================================================================================================
// K0c — chains of fixed-Huffman blocks.  A fixed-Huffman block (BTYPE=1, deflate.lisp:518-528 ->
// ht-constants.lisp:9-32) has no header to recognise, but where one FOLLOWS another the end-of-block code of the
// fixed code (seven zero bits) is followed by BFINAL and BTYPE = 01: ten bits with nine fixed.  tbz_k0c_scan finds
// that pattern (one position in 512 of random data: weak on its own); tbz_k0c_skim then decodes, without writing a
// token, the ONE block that would start at every such position and sees where it ends; a candidate is kept only if
// it is the second link of a chain: a block ends exactly on it whose own start a block ends on (tbz_k0c_link,
// tbz_k0c_filter).
// What survives joins the markers like K0b's candidates — and is used only if the block chain lands on it.
// The skim is the fixed code in arithmetic (RFC 1951 3.2.6): no tables.
// Run for streams whose items are still large after K0 and K0b (nothing was found in them).
// ================================================================================================
constexpr u32 K0C_TILE = 16u << 10;       // octets of memory per workgroup of the scan
constexpr u32 K0C_SLOTS = 512;            // pattern hits kept per 16 KiB tile (random data: ~256)
constexpr u64 K0C_MAX_BLOCK = 16u << 10;  // bits: a candidate whose block would be longer is not followed (the skim is one
                                          // lane per block: its longest block is the kernel's duration)

TBZ_KERNEL void tbz_k0c_scan(K0bParams P) {
  const u32 lane = tbz_lane();
  const u32 tile = tbz_block();
  const u32 s = k0b_find_stream(P, tile);
  const uintptr_t base = (uintptr_t)P.in_base;
  const uintptr_t s_lo = base + P.str_off[s], s_hi = s_lo + P.str_len[s];
  const uintptr_t t0 = (s_lo & ~(uintptr_t)15) + (uintptr_t)(tile - P.tile_first[s]) * K0C_TILE;
  const u64 p_min = (u64)(s_lo - base) * 8 + 8 + (P.start_bit_off ? P.start_bit_off[s] : 0u);
  const u64 p_end = (u64)(s_hi - base) * 8;
  u64* slots = P.slots + (u64)tile * P.slots_per_tile;
  u32 nout = 0;
  for (u32 r = 0; r < K0C_TILE / 1024; r++) {
    const uintptr_t c = t0 + r * 1024 + lane * 16;
    if (t0 + r * 1024 >= s_hi) break;  // wave-uniform
    u32 w[5];
    uint4 v{};
    if (c < s_hi && c + 16 > s_lo) v = *(const uint4*)c;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    w[4] = tbz_wave_shl1(v.x);
    if (lane == 63) {
      const uintptr_t cn = c + 16;
      w[4] = (cn < s_hi && cn + 16 > s_lo) ? *(const u32*)cn : 0u;
    }
    const u64 bit0 = (u64)(c - base) * 8;
    u32 cnt = 0;
    u32 m32[4];
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
      const u64 x = ((u64)w[k + 1] << 32) | w[k];
      // q .. q+6 zero (the end-of-block code), q+8 set and q+9 clear (BTYPE = 01); the header is at q+7
      const u64 z = ~x & ~(x >> 1) & ~(x >> 2) & ~(x >> 3) & ~(x >> 4) & ~(x >> 5) & ~(x >> 6);
      u32 m = (u32)(z & (x >> 8) & ~(x >> 9));
      // keep the positions whose header lies inside the stream with room for a block behind it
      u32 keep = 0;
      for (u32 t = m; t; t &= t - 1) {
        const u32 o = (u32)__builtin_ctz(t);
        const u64 p = bit0 + 32 * k + o + 7;
        if ((i64)(bit0 + 32 * k + o) >= 0 && p >= p_min && p + 20 <= p_end) keep |= 1u << o;
      }
      m32[k] = keep;
      cnt += (u32)__builtin_popcount(keep);
    }
    if (tbz_ballot(cnt != 0) == 0) continue;  // wave-uniform
    const u32 inc = wave_incl_scan_u32(cnt);
    u32 at = nout + inc - cnt;
#pragma unroll
    for (u32 k = 0; k < 4; k++)
      for (u32 t = m32[k]; t; t &= t - 1, at++)
        if (at < P.slots_per_tile) slots[at] = bit0 + 32 * k + (u32)__builtin_ctz(t) + 7;
    nout += tbz_shfl(inc, 63);
  }
  if (lane == 0) P.counts[tile] = nout < P.slots_per_tile ? nout : P.slots_per_tile;
}

// one fixed-Huffman block from bit position p on, nothing written: the bit position after its end-of-block code,
// or 0 if it is not a block (a symbol that may not be used, deflate.lisp:438,:481 / huffman-tree.lisp:172-177, or
// no end within the stream / K0C_MAX_BLOCK)
TBZ_DEV u64 k0c_skim_one(const u8* in_base, u64 p, u64 p_end, u64 max_block) {
  K0bBits b;
  const uintptr_t a0 = (uintptr_t)in_base;
  const u32 mis = (u32)(a0 & 15);
  b.w = (const u32*)(a0 - mis);
  const u64 a = p + mis * 8;
  b.nwords = (mis * 8 + p_end + 31) >> 5;
  b.wi = a >> 5;
  b.qi = ~0ull;
  b.q = uint4{};
  b.buf = 0;
  b.n = 0;
  b.pre = nullptr;
  b.pre0 = 0;
  k0b_need(b, 32);
  b.buf >>= (a & 31);
  b.n -= (u32)(a & 31);
  u64 used = 3;
  k0b_take(b, 3);  // BFINAL, BTYPE = 01 (the scan saw them)
  const u64 limit = p_end - p < max_block ? p_end - p : max_block;
  for (;;) {
    if (used + 48 > limit) return 0;
    k0b_need(b, 32);
    // codes are packed MSB first: the next nine stream bits as a number whose top bit came first
    const u32 c9 = tbz_brev32((u32)b.buf) >> 23;
    const u32 c7 = c9 >> 2, c8 = c9 >> 1;
    u32 sym, L;
    if (c7 <= 23) { sym = 256 + c7; L = 7; }
    else if (c8 <= 0xBF) { sym = c8 - 0x30; L = 8; }
    else if (c8 <= 0xC7) { sym = 280 + (c8 - 0xC0); L = 8; }
    else { sym = 144 + (c9 - 0x190); L = 9; }
    u32 nb = L;
    if (sym == 256) return p + used + 7;
    if (sym > 256) {
      if (sym > 285) return 0;
      u32 base_, X;
      len_base_extra(sym - 257, base_, X);
      const u32 ds = tbz_brev32((u32)(b.buf >> (L + X))) >> 27;  // five bits, MSB first
      if (ds > 29) return 0;
      u32 dbase, DX;
      dist_base_extra(ds, dbase, DX);
      nb = L + X + 5 + DX;  // <= 9 + 5 + 5 + 13 = 32
    }
    b.buf >>= nb;
    b.n -= nb;
    used += nb;
  }
}

// where does the block of every candidate end, and is that end a candidate too (K0C_SLOTS / 64 workgroups per tile)
TBZ_KERNEL void tbz_k0c_skim(K0bParams P) {
  const u32 lane = tbz_lane(), tile = tbz_block() / (K0C_SLOTS / 64), part = tbz_block() % (K0C_SLOTS / 64);
  const u32 s = k0b_find_stream(P, tile);
  const uintptr_t base = (uintptr_t)P.in_base;
  const uintptr_t s_lo = base + P.str_off[s];
  const uintptr_t a_lo = s_lo & ~(uintptr_t)15;  // address of the stream's first tile
  const u64 p_end = (P.str_off[s] + P.str_len[s]) * 8;
  const u64* slots = P.slots + (u64)tile * P.slots_per_tile;
  const u32 count = P.counts[tile];
  for (u32 j = part * 64 + lane; j < count; j += K0C_SLOTS) {
    const u64 p = slots[j];
    const u64 e = k0c_skim_one(P.in_base, p, p_end, P.max_block);
    P.ends[(u64)tile * P.slots_per_tile + j] = 0;
    if (!e) continue;
    // the candidate at bit e, if there is one: it lives in the tile that holds the OCTET e / 8 - 1 + ... = the pattern's
    // position e - 7 (slots are filed by where the pattern starts)
    const u64 q = e - 7;
    const uintptr_t addr = base + (q >> 3);
    if (addr < a_lo) continue;
    const u32 t2 = P.tile_first[s] + (u32)((addr - a_lo) / K0C_TILE);
    if (t2 >= P.tile_first[s + 1]) continue;
    const u64* sl2 = P.slots + (u64)t2 * P.slots_per_tile;
    u32 lo = 0, hi = P.counts[t2];
    while (lo < hi) {
      const u32 mid = (lo + hi) >> 1;
      if (sl2[mid] < e) lo = mid + 1; else hi = mid;
    }
    if (lo < P.counts[t2] && sl2[lo] == e) {
      const u64 target = (u64)t2 * P.slots_per_tile + lo;
      P.ends[(u64)tile * P.slots_per_tile + j] = ~target;        // (the slot my block ends on, for tbz_k0c_link)
      P.link[target * 2] = 1;                                     // a block ends on that candidate (racing writers write the same octet)
    }
  }
}

// second link: a candidate on which a block ends passes that on to the candidate its own block ends on
TBZ_KERNEL void tbz_k0c_link(K0bParams P) {
  const u32 tile = tbz_block();
  const u32 count = P.counts[tile];
  for (u32 j = tbz_lane(); j < count; j += 64) {
    const u64 idx = (u64)tile * P.slots_per_tile + j;
    const u64 t = P.ends[idx];
    if (t != 0 && P.link[idx * 2]) P.link[(~t) * 2 + 1] = 1;
  }
}

// keep the candidates that are part of a chain — and that satisfy the spacing rule (tbz_k0b_space: blocks of a few
// tokens are simply decoded through by the item before them).  "Slots of the list before it" are all pattern hits,
// chained or not: conservative, and immutable while this kernel runs.
TBZ_KERNEL void tbz_k0c_filter(K0bParams P) {
  const u32 lane = tbz_lane(), tile = tbz_block();
  const u32 s = k0b_find_stream(P, tile);
  const u64* slots = P.slots + (u64)tile * P.slots_per_tile;
  const u8* link = P.link + (u64)tile * P.slots_per_tile * 2;
  const u32 count = P.counts[tile];
  const u64 head = P.str_off[s] * 8 + (P.start_bit_off ? P.start_bit_off[s] : 0u);
  u64 carry = k0x_prev_tile_last(P, s, tile);
  u32 kept = 0;
  for (u32 j0 = 0; j0 < P.slots_per_tile; j0 += 64) {  // wave-uniform trip count; every mask word is written
    const u32 j = j0 + lane;
    const bool have = j < count;
    const u64 p = have ? slots[j] : 0;
    // kept: the candidates on which a block ends whose own start is one a block ends on — two links of a chain.
    // (One link happens by chance: one pattern hit in a few hundred is the end of SOME skimmed block; and that a
    // candidate's own block ends on a candidate says little: a false start inside a block falls into step with the
    // true token sequence and ends where the block ends.)
    const bool ok = have && link[2 * j + 1] != 0;
    const u64 km = tbz_ballot(k0x_spaced(P, s, head, p, have, ok, carry));
    if (lane == 0) P.keep[(u64)tile * (P.slots_per_tile / 64) + j0 / 64] = km;
    kept += tbz_popc64(km);
  }
  if (lane == 0) P.kcounts[tile] = kept;
}

// single wave: exclusive scan of the per-tile counts
// exclusive scan of the tiles' counts: ONE workgroup of 1024 threads, 1024 tiles per step (a single wave took 0.31 ms
// for the 63 000 tiles of a 1 GiB stream: one memory round trip per 64 tiles)
constexpr u32 K0B_SCAN_THREADS = 1024;
TBZ_KERNEL_WG(1024, 1) void tbz_k0b_offsets(K0bParams P) {
  TBZ_SHARED u32 wsum[16];
  const u32 lane = tbz_lane(), wave = tbz_wave(), tid = wave * 64 + lane;
  u32 carry = 0;
  for (u32 i = 0; i < P.n_tiles; i += K0B_SCAN_THREADS) {  // uniform over the workgroup
    const bool in = i + tid < P.n_tiles;
    const u32 v = in ? P.kcounts[i + tid] : 0;
    const u32 inc = wave_incl_scan_u32(v);
    if (lane == 63) wsum[wave] = inc;
    tbz_wg_barrier();
    u32 before = 0, total = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
      const u32 x = wsum[k];
      before += k < wave ? x : 0u;
      total += x;
    }
    if (in) P.offsets[i + tid] = carry + before + inc - v;
    carry += total;
    tbz_wg_barrier();  // wsum is rewritten in the next step
  }
  if (tid == 0) {
    P.offsets[P.n_tiles] = carry;
    P.head[0] = carry;
  }
}

// tile slots -> the compact candidate list; workgroup 0 writes the per-stream index
TBZ_KERNEL void tbz_k0b_compact(K0bParams P) {
  const u32 lane = tbz_lane(), t = tbz_block();
  const u32 n = P.counts[t];
  u32 o = P.offsets[t];
  for (u32 j0 = 0; j0 < n; j0 += 64) {  // the slots that passed the spacing rule (tbz_k0b_space / tbz_k0c_filter)
    const u64 km = P.keep[(u64)t * (P.slots_per_tile / 64) + j0 / 64];
    if ((km >> lane) & 1) P.cands[o + tbz_popc64(km & ((1ull << lane) - 1))] = P.slots[(u64)t * P.slots_per_tile + j0 + lane];
    o += tbz_popc64(km);
  }
  if (t == 0)
    for (u32 s = lane; s <= P.n_streams; s += 64) {
      const u32 fc = P.offsets[s < P.n_streams ? P.tile_first[s] : P.n_tiles];
      P.first_cand[s] = fc;
      P.first_merged[s] = P.first_marker[s] + fc;
      if (s == P.n_streams) {
        P.head_merged[0] = P.first_marker[s] + fc;
        P.head_merged[1] = 0;
      }
    }
}

// merge by rank: per stream both lists ascend and share no element (tbz_k0b_validate drops the block after a
// flush marker), so an element's place is its own index plus the number of smaller elements of the other list
TBZ_KERNEL void tbz_k0b_merge(K0bParams P) {
  const u32 i = tbz_block() * 64 + tbz_lane();
  const u32 n_m = P.first_marker[P.n_streams], n_c = P.first_cand[P.n_streams];
  if (i >= n_m + n_c) return;
  const bool is_m = i < n_m;
  const u32 idx = is_m ? i : i - n_m;
  const u32* first = is_m ? P.first_marker : P.first_cand;
  u32 lo = 0, hi = P.n_streams;  // stream: first[lo] <= idx < first[hi]
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (first[mid] <= idx) lo = mid; else hi = mid;
  }
  const u32 s = lo;
  const u64 v = is_m ? P.markers[idx] : P.cands[idx];
  const u64* other = is_m ? P.cands : P.markers;
  const u32* ofirst = is_m ? P.first_cand : P.first_marker;
  u32 a = ofirst[s], b = ofirst[s + 1];
  const u32 a0 = a;
  while (a < b) {
    const u32 mid = (a + b) >> 1;
    if (other[mid] < v) a = mid + 1; else b = mid;
  }
  P.merged[P.first_merged[s] + (idx - first[s]) + (a - a0)] = v;
}

// ================================================================================================
// K1 — Huffman decode to tokens, ONE LANE PER ITEM (64 independent decoders per wavefront).
//
// Why lane-per-item: symbol decode is a serial dependent chain (lookup -> shift -> lookup), so one
// decoder can use one lane.  A first version ran one decoder per WAVE; the compiler (correctly)
// scalarised it onto the CU's single scalar ALU and the kernel became SALU-bound at ~1700 cycles
// per token (profiles/r01_v1_*).  Here every lane of the 4 SIMDs' VALUs decodes its own item.
//
// Everything the token loop touches is in registers or LDS — NO global loads inside it, because
// vmcnt is a per-wave in-order counter: one lane's load makes all 64 lanes wait for every store in
// flight (measured: a full memory round trip per iteration).
//   - NO lookup tables: a fast table only pays if all 64 lanes hit it, which never happens (some lane
//     always has a long code, so the wave always runs both paths), and it costs the LDS that limits
//     occupancy.  Instead: canonical decode — the code length is 1 + #{L : r16 >= limit[L]} (fifteen
//     register compares), the symbol comes from a compact per-lane list in LDS.  31 KiB per
//     workgroup -> 5 workgroups = 320 decoders per CU
//   - compressed input: a K1_INBUF-word LDS window per lane, reloaded by all lanes together once per
//     phase of K1_PHASE tokens (nested loops make the wave reconverge at the reload)
//   - tokens are stored straight to the item's token region (consecutive u16 per lane, merged in L2);
//     stores need no wait
// Replaces deflate.lisp:518-702 + huffman-tree.lisp:99-218 (same acceptance rules and errors).
// ================================================================================================


// token words (u16):
//   0x00bb                      literal octet
//   0x8000 | (len-3)            match head, followed by  (dist-1)            (bit 15 clear)
//   0xC000 | (n & 0x3fff)       stored-run head: n octets copied verbatim from the input, followed by
//                               (n>>14) | (src&0x1fff)<<2 , (src>>13)&0x7fff , (src>>28)&0x7fff
//   0x4000                      no-op (pads a run to a multiple of 8 words)
// payload words always have bit 15 clear, so a word with bit 15 set is always a head; bit 14 of a word
// that is not a payload word marks the no-op.
constexpr u32 TOK_MATCH = 0x8000u, TOK_STORED = 0xC000u, TOK_NOP = 0x4000u;

constexpr u32 K1_SCRATCH = 512;   // octets of global scratch per item: lens[320] (code lengths while a header is parsed)
constexpr u32 K1_SC_LENS = 0;
constexpr u32 K1_INBUF = 16;      // 32-bit words of compressed input windowed per lane (64 octets); multiple of 4
constexpr u32 K1_PHASE = 32;      // tokens decoded per phase between window reloads
#ifndef TBZ_EXP_PHASE
#define TBZ_EXP_PHASE 32
#endif
constexpr u32 KG_PHASE = TBZ_EXP_PHASE;  // the same for the gang kernels' trips
constexpr u32 K1_LCAP = 288;      // every lit/len symbol (canonical order) is held in LDS per lane

// Per-workgroup LDS, every array LANE-INTERLEAVED ([index][lane]): the bank depends on the lane only, so
// 64 lanes reading 64 different indices never conflict beyond the 2-lanes-per-dword sharing of the
// narrow types.  32 KiB -> 5 workgroups (320 decoders) per CU.
struct K1Lds {
  u8 lsym8[K1_LCAP][64];        // 18 KiB   lit/len symbols in canonical order, low 8 bits
  u32 lbit8[K1_LCAP / 32][64];  // 2.25 KiB … bit 8 (end-of-block and length symbols)
  u16 ldlt[16][64];             // 2 KiB    lit/len: slot = code + ldlt[len]
  u8 dsym8[32][64];             // 2 KiB    distance symbols in canonical order (also the code-length code's)
  u16 ddlt[16][64];             // 2 KiB
  u32 inbuf[K1_INBUF][64];      // 5 KiB      per-lane window of the compressed stream; its first 4 KiB double as
                                //          the per-lane counters while a code is built (the window is reloaded after)
};
static_assert(K1_INBUF % 4 == 0 && K1_INBUF * 256 >= 4096, "window: 16-octet loads; doubles as 4 KiB of build counters");
static_assert(sizeof(K1Lds) <= 32 * 1024, "five K1 workgroups must fit one CU's 160 KiB LDS");

struct K1Params {
  const u8* in_base;
  u16* tok;       // token pool: item tokens start at tok[item.start_bit]; words written never exceed bits consumed
                  // (this kernel's items either live in a pool of one word per bit, or bring their own region: ITEM_EXPLICIT)
  const Item* items;
  SegResult* res;
  const u64* markers;
  u8* scratch;    // n_items * K1_SCRATCH octets
  RunRec* runs;   // run tables (one run per item here — the lane writes its tokens contiguously — which is SegResult::run0:
                  // the table is only named in the result)
  const u32* first_marker;  // [n_streams+1]: a stream's markers are markers[first_marker[s] .. first_marker[s+1])
  u32 n_markers;
  u32 n_items;
  u32 items_per_wg;  // 1..64: lanes >= items_per_wg idle (used to spread few large items over all CUs)
  u64 resume_bit;    // ITEM_RESUME: where the token loop of the item's first block is entered (bit position relative to in_base)
};

// per-lane bit reader (deflate.lisp:140-231 restated): LSB-first, 32-bit words, one word of lookahead.
// This is the general (64-bit position) form used for headers and block framing; the token loop works
// on a phase-local 32-bit copy.
struct BitReader {
  const u32* w;
  u32 (*buf)[64];  // this workgroup's LDS input windows, [word][lane]
  u64 nwords;      // words that contain stream octets
  u32 tail_mask;
  u32 bias;        // bits between the aligned word base and in_base (0, 8, 16, 24)
  u64 pos;         // bit position relative to in_base
  u64 wi;
  u64 bw;          // word index held in buf[0]; 2^62 (never within the window of a real index) when invalid
  u32 lo, hi, nx, o;
  u32 nw;          // words per lane in the window (K1_INBUF; the gang kernels: KG_INBUF); multiple of 4
};
TBZ_DEV u32 br_word_global(const BitReader& b, u64 i) {
  u32 v = 0;
  if (i < b.nwords) {
    v = b.w[i];
    if (i + 1 == b.nwords) v &= b.tail_mask;
  }
  return v;
}
// words come from the lane's LDS window when it covers them, else straight from memory, so
// correctness never depends on when the window was loaded
TBZ_DEV u32 br_word(const BitReader& b, u64 i) {
  u64 k = i - b.bw;
  if (k < b.nw) return b.buf[k][tbz_lane()];
  return br_word_global(b, i);
}
struct __attribute__((packed, aligned(4))) U32x4 {
  u32 a, b, c, d;
};
// reload the lane's window so that it starts at the current word (octets past the stream read as 0)
TBZ_DEV void br_refill(BitReader& b) {
  const u32 lane = tbz_lane();
  const u64 w0 = b.wi;
  if (w0 + b.nw < b.nwords) {  // whole window inside the stream, no tail masking: 16-octet loads
#pragma unroll
    for (u32 k = 0; k < K1_INBUF; k += 4) {
      if (k >= b.nw) break;
      U32x4 v = *(const U32x4*)(b.w + w0 + k);
      b.buf[k][lane] = v.a;
      b.buf[k + 1][lane] = v.b;
      b.buf[k + 2][lane] = v.c;
      b.buf[k + 3][lane] = v.d;
    }
  } else {
    for (u32 k = 0; k < b.nw; k++) b.buf[k][lane] = br_word_global(b, w0 + k);
  }
  b.bw = w0;
}
TBZ_DEV void br_init(BitReader& b, const u8* in_base, u64 end_byte, u32 (*buf)[64], u32 nw = K1_INBUF) {
  b.buf = buf;
  b.nw = nw;
  b.bw = 1ull << 62;
  uintptr_t base = (uintptr_t)in_base;
  u32 mis = (u32)(base & 3);
  b.w = (const u32*)(base - mis);
  b.bias = mis * 8;
  u64 endb = mis + end_byte;
  b.nwords = (endb + 3) >> 2;
  u32 tail = (u32)(endb & 3);
  b.tail_mask = tail ? ((1u << (8 * tail)) - 1) : 0xFFFFFFFFu;
}
TBZ_DEV void br_seek(BitReader& b, u64 pos) {
  u64 a = pos + b.bias;
  b.pos = pos;
  b.wi = a >> 5;
  b.o = (u32)(a & 31);
  b.lo = br_word(b, b.wi);
  b.hi = br_word(b, b.wi + 1);
  b.nx = br_word(b, b.wi + 2);
}
TBZ_DEV u32 br_peek(const BitReader& b) { return tbz_alignbit(b.hi, b.lo, b.o); }
TBZ_DEV void br_skip(BitReader& b, u32 n) {  // n <= 32
  b.o += n;
  b.pos += n;
  if (b.o >= 32) {
    b.o -= 32;
    b.lo = b.hi;
    b.hi = b.nx;
    b.wi += 1;
    b.nx = br_word(b, b.wi + 2);
  }
}

// Canonical code of one alphabet, per lane.  lim[L-1] = (first code of length L + number of codes of
// length L) left-aligned to 16 bits; the sequence is non-decreasing in L, so for the first 16 stream
// bits r16 (MSB-first) the code length is 1 + #{L : r16 >= lim[L-1]} — fifteen compares, no table.
// 16 means "no code starts like this" (a hole of an incomplete code, or an empty alphabet).
struct Canon {
  u32 lim[15];
  u32 min_len;  // shortest code length = width of the reference's root table (huffman-tree.lisp:144)
};

// where an alphabet's per-lane decode data lives (all LDS except the overflow list)
struct CanonStore {
  u16 (*dlt)[64];   // [16][64]: slot in canonical order = (code of length L) + dlt[L]   (mod 2^16)
  u8 (*sym8)[64];   // [cap][64]: low 8 bits of the symbol at each slot
  u32 (*bit8)[64];  // [cap/32][64]: bit 8 of the symbol at each slot (null: symbols < 256)
  u32 cap;          // slots; covers the whole alphabet (288 / 32)
};

// Per-lane canonical-Huffman build.  `lens` (global scratch) holds n code lengths 0..15.
// Acceptance rules of build-tree-part (huffman-tree.lisp:112-122): over-subscribed -> error;
// incomplete -> error unless at most one symbol is coded; all-zero -> every pattern is a hole.
TBZ_DEV i32 build_canon(const u8* lens, u32 n, u16 (*tmp)[64], const CanonStore& cs, Canon& cn) {
  const u32 lane = tbz_lane();
#pragma unroll
  for (int L = 0; L < 16; L++) tmp[L][lane] = 0;
  for (u32 i = 0; i < n; i++) {
    u32 l = lens[i];
    if (l) tmp[l][lane] = (u16)(tmp[l][lane] + 1);
  }
  u32 used = 0, code = 0, off = 0, prev = 0;
  i32 left = 1, err = 0;
  cn.min_len = 0;
#pragma unroll
  for (int L = 1; L < 16; L++) {
    u32 c = tmp[L][lane];
    left <<= 1;
    if ((i32)c > left && !err) err = E_OVERSUB;
    left -= (i32)c;
    used += c;
    if (c && !cn.min_len) cn.min_len = L;
    code = (code + prev) << 1;  // first canonical code of length L
    prev = c;
    tmp[L][lane] = (u16)off;            // next free slot in canonical order
    cs.dlt[L][lane] = (u16)(off - code);
    cn.lim[L - 1] = (code + c) << (16 - L);
    off += c;
  }
  if (!err && left > 0 && used > 1) err = E_INCOMPLETE;
  // one code alone, 11 bits or longer: the reference's root table of 2^length entries does not fit its node array
  // (huffman-tree.lisp:213-217 against constants.lisp:4-7) and the build fails.  Only this shape is mirrored here: the
  // array's other bounds (nested sub-tables past 1444 entries in all, one starting past entry 1023) are the oracle's
  // to report, and no stream of the suite reaches them, the deepest codes of case_code_tables included
  if (!err && used == 1 && cn.min_len > 10) err = E_TREE_OVERFLOW;
  if (err) return err;
  if (cs.bit8)
    for (u32 k = 0; k < cs.cap / 32; k++) cs.bit8[k][lane] = 0;
  for (u32 i = 0; i < n; i++) {
    u32 l = lens[i];
    if (!l) continue;
    u32 slot = tmp[l][lane];
    tmp[l][lane] = (u16)(slot + 1);
    cs.sym8[slot][lane] = (u8)i;  // slot < n <= cap
    if (i >= 256) cs.bit8[slot >> 5][lane] |= 1u << (slot & 31);
  }
  return 0;
}

// decode one symbol from the 32 bits `pk` (LSB-first stream order).  Returns the code length (16 =
// hole) and the symbol.
TBZ_DEV u32 canon_decode(u32 pk, const Canon& cn, const CanonStore& cs, u32& sym) {
  const u32 lane = tbz_lane();
  u32 r16 = tbz_brev32(pk) >> 16;
  u32 L = 1;
#pragma unroll
  for (int k = 0; k < 15; k++) L += r16 >= cn.lim[k] ? 1u : 0u;
  u32 slot = ((r16 >> (16 - (L & 15))) + cs.dlt[L & 15][lane]) & 0xffff;
  slot = slot < cs.cap ? slot : 0;  // only a hole (L = 16) can point outside; its symbol is never used
  u32 s = cs.sym8[slot][lane];
  if (cs.bit8) s |= ((cs.bit8[slot >> 5][lane] >> (slot & 31)) & 1u) << 8;
  sym = s;
  return L;
}

struct K1State {
  BitReader br;
  u64 end_bit, limit_bit;
  u64 produced;  // octets the tokens emitted so far produce
  u64 fail_pos;  // bit position reported on underrun / overshoot
  u16* tok;      // next token word of this item
  u16* tok0;
  u32 deficit;
  u32 hist0;     // octets of the stream before this item, when the host knows (ITEM_HIST; else 0): with it the
  u64 viol_out;  // first match that reaches before the stream's start is located exactly (octets into the item)
};

// availability / landing-limit test after consuming bits for a token or header field that started
// at `p0`.  Underrun wins (deflate.lisp:399-427: the whole symbol is pushed back and re-read).
#define K1_CHECK(p0)                 \
  do {                               \
    if (st.br.pos > st.end_bit) {    \
      st.fail_pos = (p0);            \
      return SEG_UNDERRUN;           \
    }                                \
    if (st.br.pos > st.limit_bit) {  \
      st.fail_pos = (p0);            \
      return SEG_OVERSHOOT;          \
    }                                \
  } while (0)

struct K1Tables {
  Canon ll;  // literal/length alphabet
  Canon ld;  // distance alphabet
};
TBZ_DEV u16 (*k1_tmp(K1Lds& S))[64] { return (u16(*)[64])S.inbuf; }
TBZ_DEV CanonStore k1_cs_lit(K1Lds& S, u8*) {
  return CanonStore{S.ldlt, S.lsym8, S.lbit8, K1_LCAP};
}
TBZ_DEV CanonStore k1_cs_dist(K1Lds& S) { return CanonStore{S.ddlt, S.dsym8, nullptr, 32}; }

// fixed (BTYPE=1) code lengths: huffman-tree.lisp:89-97
TBZ_DEV i32 k1_build_fixed(K1Lds& S, K1State& st, K1Tables& T, u8* sc) {
  st.br.bw = 1ull << 62;  // the builders use the window's LDS as scratch
  u8* lens = sc + K1_SC_LENS;
  for (u32 i = 0; i < 320; i++) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
  i32 e = build_canon(lens, 288, k1_tmp(S), k1_cs_lit(S, sc), T.ll);
  if (e) return e;
  return build_canon(lens + 288, 32, k1_tmp(S), k1_cs_dist(S), T.ld);
}

// :dynamic-huffman-block … :dht-len-table-data (deflate.lisp:577-669)
// `sizes` != nullptr: stop once the code lengths are in `sc` and report hlit | hdist << 16 there (K1h)
TBZ_DEV i32 k1_dynamic_header(K1Lds& S, K1State& st, K1Tables& T, u8* sc, u32* sizes = nullptr) {
  const u64 p0 = st.br.pos;
  u32 pk = br_peek(st.br);
  u32 hlit = (pk & 31) + 257, hdist = ((pk >> 5) & 31) + 1, hclen = ((pk >> 10) & 15) + 4;
  br_skip(st.br, 14);
  K1_CHECK(p0);
  u8* lens = sc + K1_SC_LENS;
  for (u32 i = 0; i < 19; i++) lens[i] = 0;
  for (u32 i = 0; i < hclen; i++) {
    u32 v = br_peek(st.br) & 7;
    br_skip(st.br, 3);
    lens[c_cl_order[i]] = (u8)v;
  }
  K1_CHECK(p0);
  // the window's LDS is scratch for the table builds below: carry on from registers/memory (a header
  // is ~60 octets) and let the token loop reload it.  The code-length code borrows the distance
  // alphabet's LDS (the distance code is built after the lengths are read).
  st.br.bw = 1ull << 62;
  Canon ccl;
  const CanonStore cscl = k1_cs_dist(S);
  i32 e = build_canon(lens, 19, k1_tmp(S), cscl, ccl);
  if (e) return e;
  const u32 n = hlit + hdist;
  u32 i = 0, last = 0xff;
  while (i < n) {
    const u64 ps = st.br.pos;
    pk = br_peek(st.br);
    u32 sym;
    u32 L = canon_decode(pk, ccl, cscl, sym);
    if (L > 15) {  // unassigned pattern: error unless the input ends inside the root index
      if (st.br.pos + ccl.min_len > st.end_bit) {
        st.fail_pos = ps;
        return SEG_UNDERRUN;
      }
      return E_INVALID_CODE;
    }
    u32 xb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
    u32 x = tbz_bfe(pk, L, xb);
    br_skip(st.br, L + xb);
    K1_CHECK(ps);
    if (sym < 16) {
      lens[i++] = (u8)sym;
      last = sym;
    } else {
      u32 rep, val;
      if (sym == 16) {
        if (last >= 16) return E_REPEAT_NO_PREV;
        rep = 3 + x;
        val = last;
      } else {
        rep = (sym == 17 ? 3 : 11) + x;
        val = 0;
        last = 0;
      }
      if (i + rep > n) return E_REPEAT_OVERRUN;
      for (u32 k = 0; k < rep; k++) lens[i + k] = (u8)val;
      i += rep;
    }
  }
  if (sizes) {
    *sizes = hlit | (hdist << 16);
    return 0;
  }
  e = build_canon(lens, hlit, k1_tmp(S), k1_cs_lit(S, sc), T.ll);
  if (e) return e;
  return build_canon(lens + hlit, hdist, k1_tmp(S), k1_cs_dist(S), T.ld);
}

// :decode-compressed-data (deflate.lisp:673-702): returns 0 at end-of-block.
//
// Structure: phases.  A phase reloads the lane's LDS input window at the current position and then
// decodes at most K1_PHASE tokens out of it with 32-bit phase-local state.  The two loops are nested ON
// PURPOSE: the wave reconverges at the reload, so the 64 lanes reload together instead of one lane or
// other stalling the wave on memory every iteration; and a phase is bounded by an iteration count (the
// window is sized so that few lanes run out earlier), so lanes do not idle waiting for the slowest
// consumer of bits.
TBZ_DEV i32 k1_decode_block(K1Lds& S, K1State& st, const K1Tables& T, u8* sc) {
  const u32 lane = tbz_lane();
  const CanonStore csl = k1_cs_lit(S, sc), csd = k1_cs_dist(S);
  enum { RUN = 0, DONE_EOB, FAIL_LIMIT, FAIL_CODE_LIT, FAIL_CODE_DIST, FAIL_SYM };
  for (;;) {
    br_refill(st.br);
    BitReader& B = st.br;
    u32 lo = B.lo, hi = B.hi, nx = B.nx, o = B.o;
    u32 k = 3;  // window slot of the word after nx
    // bits this item may still consume before underrun / overshoot (saturated; a phase uses < 2^12)
    u64 lim64 = st.end_bit < st.limit_bit ? st.end_bit : st.limit_bit;
    i32 rem = lim64 <= B.pos ? 0 : ((lim64 - B.pos) > 0x7fffff00ull ? 0x7fffff00 : (i32)(lim64 - B.pos));
    const i32 rem_start = rem;
    i32 rem_tok = rem;  // value of rem when the current token started
    const u64 hist64 = st.produced + st.hist0;
    u32 hist = hist64 > 32768 ? 32768u : (u32)hist64;  // history available to this item (saturated)
    u32 prod = 0;       // octets produced in this phase
    u32 deficit = st.deficit;
    u16* tp = st.tok;
    u32 why = RUN;

// branch-free: the next window word is read every time and selected in when a word boundary is crossed
#define K1_SKIP(n)                   \
  do {                               \
    o += (n);                        \
    rem -= (i32)(n);                 \
    const u32 nw_ = B.buf[k][lane];  \
    const bool ge_ = o >= 32;        \
    o = ge_ ? o - 32 : o;            \
    lo = ge_ ? hi : lo;              \
    hi = ge_ ? nx : hi;              \
    nx = ge_ ? nw_ : nx;             \
    k += ge_ ? 1u : 0u;              \
  } while (0)

    for (u32 it = 0; it < K1_PHASE && k < K1_INBUF - 3; it++) {  // a token takes at most 3 window words
      rem_tok = rem;
      u32 pk = tbz_alignbit(hi, lo, o);
      u32 sym;
      u32 L = canon_decode(pk, T.ll, csl, sym);
      if (L > 15) {
        why = FAIL_CODE_LIT;
        break;
      }
      if (sym < 256) {
        K1_SKIP(L);
        if (rem < 0) { why = FAIL_LIMIT; break; }
        *tp++ = (u16)sym;
        prod += 1;
      } else if (sym == 256) {  // end of block
        K1_SKIP(L);
        if (rem < 0) { why = FAIL_LIMIT; break; }
        why = DONE_EOB;
        break;
      } else {
        if (sym > 285) {  // 286/287 are coded but may not be used (huffman-tree.lisp:176-177)
          K1_SKIP(L);
          why = rem < 0 ? FAIL_LIMIT : FAIL_SYM;
          break;
        }
        u32 base, X;
        len_base_extra(sym - 257, base, X);
        u32 len = base + tbz_bfe(pk, L, X);
        K1_SKIP(L + X);
        u32 pd = tbz_alignbit(hi, lo, o);
        u32 ds;
        u32 DL = canon_decode(pd, T.ld, csd, ds);
        if (DL > 15) {
          why = FAIL_CODE_DIST;
          break;
        }
        if (ds > 29) {  // 30/31 (huffman-tree.lisp:172-175)
          K1_SKIP(DL);
          why = rem < 0 ? FAIL_LIMIT : FAIL_SYM;
          break;
        }
        u32 dbase, DX;
        dist_base_extra(ds, dbase, DX);
        u32 dist = dbase + tbz_bfe(pd, DL, DX);
        K1_SKIP(DL + DX);
        if (rem < 0) { why = FAIL_LIMIT; break; }
        u32 h = hist + prod;
        h = h > 32768 ? 32768 : h;
        if (dist > h) {
          u32 d = dist - h;
          deficit = d > deficit ? d : deficit;
          if (st.viol_out == ~0ull) st.viol_out = st.produced + prod;
        }
        tp[0] = (u16)(TOK_MATCH | (len - 3));
        tp[1] = (u16)(dist - 1);
        tp += 2;
        prod += len;
      }
    }
#undef K1_SKIP
    // ---- write the phase back into the 64-bit state
    u32 used = (u32)(rem_start - rem);      // bits consumed in this phase (also counts the failed token's)
    u32 tok_bits = (u32)(rem_tok - rem);    // … of which belong to the token in flight at a failure
    B.pos += used;
    B.wi += k - 3;
    B.lo = lo;
    B.hi = hi;
    B.nx = nx;
    B.o = o;
    st.tok = tp;
    st.produced += prod;
    st.deficit = deficit;
    if (why == RUN) continue;  // phase over: reload and go on
    if (why == DONE_EOB) return 0;
    const u64 p0 = B.pos - tok_bits;  // where the failing token started
    if (why == FAIL_LIMIT) {
      st.fail_pos = p0;
      return B.pos > st.end_bit ? SEG_UNDERRUN : SEG_OVERSHOOT;
    }
    if (why == FAIL_SYM) return E_INVALID_CODE;
    // an unassigned bit pattern: error unless the input ends inside the bits the reference would need
    u32 bad_bits = why == FAIL_CODE_LIT ? T.ll.min_len : T.ld.min_len;
    if (B.pos + bad_bits > st.end_bit) {
      st.fail_pos = p0;
      return SEG_UNDERRUN;
    }
    return E_INVALID_CODE;
  }
}

// reflected CRC-32 of one octet, bitwise (only for the optional gzip header crc16, gzip.lisp:244-255)
TBZ_DEV u32 crc_bitwise(u32 crc, u32 byte) {
  crc ^= byte;
  for (int k = 0; k < 8; k++) crc = (crc & 1) ? (0xedb88320u ^ (crc >> 1)) : (crc >> 1);
  return crc;
}
// keep the reader's LDS window over the position (a loop of k1_byte over a long field would otherwise fetch every word
// from memory on its own: one round trip per four octets)
TBZ_DEV void k1_window(BitReader& b) {
  if (b.wi + 4 > b.bw + b.nw) br_refill(b);
}
TBZ_DEV i32 k1_byte(K1State& st, u32* out, u64 p0) {
  *out = br_peek(st.br) & 0xff;
  br_skip(st.br, 8);
  if (st.br.pos > st.end_bit) {
    st.fail_pos = p0;
    return SEG_UNDERRUN;
  }
  return 0;
}
// container headers: zlib.lisp:14-37,:110-128  gzip.lisp:113-266
// crc_tab: the 256-entry table of checksums.lisp:177-193 in LDS, or nullptr (bit by bit: 40 dependent operations per
// octet — a false `1f 8b 08` candidate with FHCRC and FEXTRA set and 34 551 for a length kept ONE lane busy for 11.5 ms);
// defer_hcrc: a header with FHCRC is not parsed at all (K1h: the gang kernel does it, with the table): returns 99
// pre: the extra field's raw CRC (register starting at 0) and x^(8 * XLEN), computed by the whole gang (kg_extra_crc)
struct GzExtraCrc {
  u32 valid, raw, xpow;
};
TBZ_DEV u32 crc_mulmod(u32 a, u32 b);
TBZ_DEV i32 k1_container_header(K1State& st, u32 fmt, const u32* crc_tab = nullptr, bool defer_hcrc = false,
                                const GzExtraCrc* pre = nullptr) {
  const u64 p0 = st.br.pos;
  i32 e;
  u32 b0, b1, t;
  if (fmt == 1) {
    if ((e = k1_byte(st, &b0, p0))) return e;
    if ((e = k1_byte(st, &b1, p0))) return e;
    if (((b0 * 256 + b1) % 31) != 0) return E_ZLIB_HEADER;
    if ((b0 & 15) != 8) return E_ZLIB_HEADER;
    if ((b0 >> 4) > 7) return E_ZLIB_HEADER;
    if (b1 & 0x20) return E_ZLIB_DICT;
    return 0;
  }
  if (fmt == 2) {
    u32 crc = 0xffffffffu;
    u32 flg = 0;
    auto crc_step = [&](u32 c, u32 b) { return crc_tab ? (c >> 8) ^ crc_tab[(c ^ b) & 0xffu] : crc_bitwise(c, b); };
    for (int i = 0; i < 10; i++) {
      // the reference takes ID1+ID2 and CM+FLG as pairs: 16 bits or input-underrun, before it looks at either
      // octet (gzip.lisp:113-131)
      if ((i == 0 || i == 2) && st.br.pos + 16 > st.end_bit) {
        st.fail_pos = p0;
        return SEG_UNDERRUN;
      }
      if ((e = k1_byte(st, &t, p0))) return e;
      crc = crc_bitwise(crc, t);
      if (i == 0 && t != 0x1f) return E_GZIP_MAGIC;
      if (i == 1 && t != 0x8b) return E_GZIP_MAGIC;
      if (i == 2 && t != 8) return E_GZIP_METHOD;
      if (i == 3) {
        flg = t;
        if (flg >> 5) return E_GZIP_FLAGS;
        if (defer_hcrc && (flg & 2)) return 99;
      }
    }
    const bool want_crc = (flg & 2) != 0;  // the header CRC is only looked at when FHCRC says there is one
    if (flg & 4) {
      if ((e = k1_byte(st, &b0, p0))) return e;
      if ((e = k1_byte(st, &b1, p0))) return e;
      crc = crc_bitwise(crc_bitwise(crc, b0), b1);
      u32 xlen = b0 | (b1 << 8);
      if (!want_crc) {
        // nobody reads the extra field here (the host has it: tbz_gzip_header_parse): step over it.  (Octet by octet
        // with a bitwise CRC this was 10+ ms for ONE lane whenever a false `1f 8b 08` candidate — compressed data —
        // happened to have FEXTRA set and 60 000 for a length.)
        if (st.br.pos + 8ull * xlen > st.end_bit) {
          st.fail_pos = p0;
          return SEG_UNDERRUN;
        }
        br_seek(st.br, st.br.pos + 8ull * xlen);
      } else if (pre && pre->valid && st.br.pos + 8ull * xlen <= st.end_bit) {
        crc = crc_mulmod(pre->xpow, crc) ^ pre->raw;  // r(A || B) = Z^|B| r(A) ^ r(B), as K5 combines its chunks
        br_seek(st.br, st.br.pos + 8ull * xlen);
      } else {
        for (u32 i = 0; i < xlen; i++) {
          k1_window(st.br);
          if ((e = k1_byte(st, &t, p0))) return e;
          crc = crc_step(crc, t);
        }
      }
    }
    for (u32 f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
      if (flg & f) {
        for (;;) {
          k1_window(st.br);
          if ((e = k1_byte(st, &t, p0))) return e;
          if (want_crc) crc = crc_step(crc, t);
          if (t == 0) break;
        }
      }
    }
    if (flg & 2) {
      if ((e = k1_byte(st, &b0, p0))) return e;
      if ((e = k1_byte(st, &b1, p0))) return e;
      if ((b0 | (b1 << 8)) != ((crc ^ 0xffffffffu) & 0xffff)) return E_GZIP_HCRC;
    }
    return 0;
  }
  return 0;
}

TBZ_KERNEL void tbz_k1_huff_decode(K1Params P) {
  TBZ_SHARED K1Lds S;
  const u32 lane = tbz_lane();
  const u32 idx = tbz_block() * P.items_per_wg + lane;
  if (lane >= P.items_per_wg || idx >= P.n_items) return;  // no collectives below: lanes are independent
  const Item it = P.items[idx];
  const u32 fmt = (it.flags >> ITEM_FMT_SHIFT) & 3;
  const bool fixup = (it.flags & ITEM_FIXUP) != 0;
  u8* sc = P.scratch + (u64)idx * K1_SCRATCH;
  K1State st;
  K1Tables T;
  br_init(st.br, P.in_base, it.end_byte, S.inbuf);
  br_seek(st.br, it.start_bit);
  st.end_bit = it.end_byte * 8;
  st.limit_bit = fixup ? ~0ull : it.limit_bit;
  st.produced = 0;
  st.deficit = 0;
  // token base: the 8-word granule of the start (fix-up items start mid-octet)
  st.tok0 = (it.flags & ITEM_EXPLICIT) ? (u16*)it.tok : P.tok + (it.start_bit & ~7ull);
  st.tok = st.tok0;
  st.fail_pos = it.start_bit;
  st.hist0 = it.flags >> ITEM_HIST_SHIFT;
  st.viol_out = ~0ull;

  i32 status = 0;
  u32 land = 0xFFFFFFFFu, tr0 = 0, tr1 = 0, tr_have = 0;
  u64 blk_pos = it.start_bit, blk_prod = 0, blk_tok = 0;
  u32 cut = 0;  // 2: ran out of input inside a stored block's payload
  int tables = 0;  // 0 none, 1 fixed, 2 dynamic

  if (it.flags & ITEM_HEAD) {
    status = k1_container_header(st, fmt);
    // the first block may itself be a candidate (K0b): the head item is the container header alone
    if (status == 0 && !fixup && st.br.pos == st.limit_bit) status = SEG_LANDED;
  }

  while (status == 0) {
    blk_pos = st.br.pos;
    blk_prod = st.produced;
    blk_tok = (u64)(st.tok - st.tok0);
    u32 pk = br_peek(st.br);
    br_skip(st.br, 3);
    if (st.br.pos > st.end_bit) { st.fail_pos = blk_pos; status = SEG_UNDERRUN; break; }
    if (st.br.pos > st.limit_bit) { status = SEG_OVERSHOOT; break; }
    const u32 bfinal = pk & 1, btype = (pk >> 1) & 3;
    if (btype == 0) {  // :uncompressed-block / :copy-block (deflate.lisp:532-573)
      br_skip(st.br, (u32)((0 - st.br.pos) & 7));
      const u64 ph = st.br.pos;
      u32 ln = br_peek(st.br);
      br_skip(st.br, 32);
      if (st.br.pos > st.end_bit) { st.fail_pos = ph; status = SEG_UNDERRUN; break; }
      u32 LEN = ln & 0xffff, NLEN = ln >> 16;
      if (NLEN != ((~LEN) & 0xffff)) { status = E_STORED_LEN; break; }
      u64 byte0 = st.br.pos >> 3;
      if ((byte0 + LEN) * 8 > st.limit_bit) { status = SEG_OVERSHOOT; break; }
      u64 avail = it.end_byte - byte0;
      u32 ncopy = avail < LEN ? (u32)avail : LEN;
      if (ncopy) {  // one stored-run token: K2 copies the octets straight from the input
        st.tok[0] = (u16)(TOK_STORED | (ncopy & 0x3fff));
        st.tok[1] = (u16)((ncopy >> 14) | ((u32)(byte0 & 0x1fff) << 2));
        st.tok[2] = (u16)((byte0 >> 13) & 0x7fff);
        st.tok[3] = (u16)((byte0 >> 28) & 0x7fff);
        st.tok += 4;
        st.produced += ncopy;
      }
      if (ncopy < LEN) { st.fail_pos = (byte0 + ncopy) * 8; status = SEG_UNDERRUN; cut = 2; break; }
      br_seek(st.br, (byte0 + LEN) * 8);
    } else if (btype == 3) {
      status = E_BTYPE;  // deflate.lisp:521
      break;
    } else {
      if (btype == 1) {
        if (tables != 1) {
          status = k1_build_fixed(S, st, T, sc);
          tables = 1;
        }
      } else {
        status = k1_dynamic_header(S, st, T, sc);
        tables = 2;
      }
      if (status) break;
      if ((it.flags & ITEM_RESUME) && blk_pos == it.start_bit && P.resume_bit > st.br.pos) br_seek(st.br, P.resume_bit);
      status = k1_decode_block(S, st, T, sc);
      if (status) break;
    }
    // :block-end (deflate.lisp:719-722)
    if (bfinal) {
      status = SEG_FINAL;
      br_skip(st.br, (u32)((0 - st.br.pos) & 7));  // byte-align (zlib.lisp:138, gzip.lisp:271)
      if (fmt == 1) {                               // adler32, big-endian (zlib.lisp:86-90)
        if (st.br.pos + 32 <= st.end_bit) {
          u32 v = br_peek(st.br);
          br_skip(st.br, 32);
          tr0 = (v >> 24) | ((v >> 8) & 0xff00) | ((v << 8) & 0xff0000) | (v << 24);
          tr_have = 2;
        }
      } else if (fmt == 2) {  // crc32 then ISIZE, little-endian (gzip.lisp:82-106)
        if (st.br.pos + 32 <= st.end_bit) {
          tr0 = br_peek(st.br);
          br_skip(st.br, 32);
          tr_have = 1;
          if (st.br.pos + 32 <= st.end_bit) {
            tr1 = br_peek(st.br);
            br_skip(st.br, 32);
            tr_have = 2;
          }
        }
      } else {
        tr_have = 2;
      }
      break;
    }
    if (!fixup) {
      if (st.br.pos == st.limit_bit) { status = SEG_LANDED; break; }
    } else {
      u64 b = st.br.pos;
      u32 lo = P.first_marker[it.stream];
      const u32 hi0 = P.first_marker[it.stream + 1];
      u32 hi = hi0;
      while (lo < hi) {
        u32 mid = (lo + hi) >> 1;
        if (P.markers[mid] < b) lo = mid + 1; else hi = mid;
      }
      if (lo < hi0 && P.markers[lo] == b) { land = lo; status = SEG_LANDED; break; }
    }
  }

  SegResult r;
  u64 TW;
  if (status == SEG_OVERSHOOT) {
    r.end_bit = blk_pos;
    r.out_bytes = blk_prod;
    TW = blk_tok;
  } else {
    r.end_bit = (status == SEG_UNDERRUN) ? st.fail_pos : st.br.pos;
    r.out_bytes = st.produced;
    TW = (u64)(st.tok - st.tok0);
  }
  // one run: pad it to the 8-word granule (the padding stays inside the item's own token region: an
  // item consumes at least 7 bits more than it has token words)
  const u64 T8 = (TW + 7) >> 3;
  for (u64 k = TW; k < T8 * 8; k++) st.tok0[k] = (u16)TOK_NOP;
  r.run0.off8 = 0;
  r.run0.n8 = (u32)T8;
  r.run0.out = r.out_bytes > 0xfffffffeull ? 0xffffffffu : (u32)r.out_bytes;
  r.run0.mdef = st.deficit;
  r.tok = (u64)st.tok0;
  r.runs = (u64)(P.runs + (it.start_bit >> RUN_SHIFT));
  r.tok_words = T8 * 8;
  r.n_runs = T8 ? 1u : 0u;
  r.pad = (status == SEG_UNDERRUN && st.fail_pos == blk_pos) ? 1u : status == SEG_UNDERRUN ? cut : 0u;
  r.status = status;
  r.max_deficit = st.deficit;
  r.trailer0 = tr0;
  r.trailer1 = tr1;
  r.trailer_have = tr_have;
  r.land_marker = land;
  r.reserved = st.viol_out;  // (the gang kernel keeps its diagnostics here)
  if (status == SEG_UNDERRUN && !(it.flags & ITEM_PROBE)) {
    // where a resumed decode would start: the block in which the input ran out, and what came out before it
    r.trailer0 = (u32)blk_pos;
    r.trailer1 = (u32)(blk_pos >> 32);
    r.reserved = blk_prod;
    r.land_marker = 0;  // 0: exact
  }
  P.res[idx] = r;
}
// K1h — header pre-pass for the gang kernel.  Parsing a dynamic block's code lengths is a serial job for ONE
// lane; inside the gang kernel that is the gang leader alone, i.e. 2 of a wave's 64 lanes busy for ~17 % of
// the kernel's instructions.  Here every lane parses the FIRST block header of its own item (64 per wave),
// leaves the code lengths in the item's scratch and the sizes / positions in a HdrRec; the gang kernel picks
// them up and goes straight to the (gang-parallel) build.  Anything unusual (not a dynamic block, error,
// underrun, limit) is simply not recorded: the gang kernel then parses that header itself, with the exact
// failure rules.
struct HdrRec {
  u64 hdr_bit;   // position of the block's 3 header bits
  u64 end_bit;   // position after the code lengths
  u32 sizes;     // hlit | hdist << 16; 0 = nothing recorded
  u32 pad;
};
struct K1hParams {
  const u8* in_base;
  const Item* items;
  u8* scratch;   // n_items * K1_SCRATCH: the code lengths
  HdrRec* hdr;
  u32 n_items;
};
TBZ_KERNEL void tbz_k1h_headers(K1hParams P) {
  TBZ_SHARED K1Lds S;
  const u32 lane = tbz_lane();
  const u32 idx = tbz_block() * 64 + lane;
  if (idx >= P.n_items) return;  // no collectives below: lanes are independent
  const Item it = P.items[idx];
  const u32 fmt = (it.flags >> ITEM_FMT_SHIFT) & 3;
  K1State st;
  K1Tables T;
  br_init(st.br, P.in_base, it.end_byte, S.inbuf);
  br_seek(st.br, it.start_bit);
  st.end_bit = it.end_byte * 8;
  st.limit_bit = (it.flags & ITEM_FIXUP) ? ~0ull : it.limit_bit;
  st.produced = 0;
  st.deficit = 0;
  st.hist0 = 0;
  st.viol_out = ~0ull;
  st.tok0 = st.tok = nullptr;
  st.fail_pos = it.start_bit;
  HdrRec h;
  h.hdr_bit = h.end_bit = 0;
  h.sizes = 0;
  h.pad = 0;
  i32 status = 0;
  if (it.flags & ITEM_HEAD) status = k1_container_header(st, fmt, nullptr, true);
  if (status == 0) {
    h.hdr_bit = st.br.pos;
    const u32 pk = br_peek(st.br);
    br_skip(st.br, 3);
    if (st.br.pos <= st.end_bit && st.br.pos <= st.limit_bit && ((pk >> 1) & 3) == 2) {
      u32 sizes = 0;
      if (k1_dynamic_header(S, st, T, P.scratch + (u64)idx * K1_SCRATCH, &sizes) == 0) {
        h.end_bit = st.br.pos;
        h.sizes = sizes;
      }
    }
  }
  P.hdr[idx] = h;
}
#undef K1_CHECK

// ================================================================================================
// K1g — Huffman decode to tokens, a GANG of G lanes per item (intra-block parallel decode).
//
// With one lane per item, K1's run time is one item's serial chain of ~1.1 us per token, and a lane
// cannot afford lookup tables (64 private tables do not fit the LDS).  Here G lanes share one item
// and ONE set of tables in the gang's LDS:
//   * the gang leader parses the block header (code lengths decoded through a 7-bit table);
//   * all G lanes build the canonical codes together (per-lane symbol chunks, packed 16-bit
//     counters, a gang prefix sum for the canonical ranks) and fill direct-lookup tables
//     (KG_TBL-bit for literal/length, KG_TBD-bit for distance; longer codes take a compare-count
//     path over the few remaining limits);
//   * the block is decoded in ROUNDS: lane g speculatively decodes the sub-range
//     [P + g*SUB, P + (g+1)*SUB) of the bitstream, starting OVL bits early so that — Huffman codes
//     being self-synchronising — it is almost always on a true token boundary by the time its
//     sub-range begins.  A lane's tokens count only if it started recording exactly where its
//     predecessor stopped (start_g == end_{g-1}; lane 0 starts at the known-good P): that equality
//     is exact, a lane that starts at a true boundary decodes the true sequence, so there are no
//     false positives.  The valid prefix of lanes is committed (token runs compacted from the
//     position-addressed staging pool into the item's contiguous token stream — K2 and the host see
//     exactly what the lane-per-item kernel produces), P moves to the last valid lane's end, and the
//     next round starts.  A mis-synchronised lane only shortens a round.
// SUB adapts to what is left of the item (the next marker is where the segment is expected to end),
// so a 16 KiB-segment item is one round.
// ================================================================================================
constexpr u32 KG_TBL = 9;               // index bits of the literal/length lookup table (first level)
constexpr u32 KG_TBD = 8;               // index bits of the distance lookup table (first level)
// second-level entries (codes longer than the index); zlib's ENOUGH bound is 340.  If a code needs more, ALL its long codes
// take the exact (slow) step instead (case_deep_codes).  Gangs of 32 — two gangs' tables per workgroup — have smaller pools
// since round 4: the 16 KiB segments they decode have shallow codes (60 - 200 / 8 - 40 entries), and the 768 octets are what
// lets sixteen workgroups share a CU's LDS; the gangs of 64 decode whole zlib blocks (codes of up to 15 bits) and keep 352 / 128
#ifndef TBZ_EXP_LPOOL32
#define TBZ_EXP_LPOOL32 288
#endif
#ifndef TBZ_EXP_DPOOL32
#define TBZ_EXP_DPOOL32 64
#endif
template <int G>
struct KgPools {
  static constexpr u32 L = G == 32 ? TBZ_EXP_LPOOL32 : 352, D = G == 32 ? TBZ_EXP_DPOOL32 : 128;
};
// words of the per-lane input window: twelve for the gangs of 32 (with their canonical lists parked in memory: 9.9 KB,
// sixteen workgroups per CU), K1_INBUF for the others.  Measured (round 4, K1 ms on config 3 / the 64 MiB no-flush stream,
// gangs of 64): 12 words + lists in memory 2.80 / 0.71; 16 words 2.59 / 0.70; lists in LDS 2.62 / 0.70; both 2.53 / 0.70 —
// a gang of 64 has ONE set of tables per workgroup and fits sixteen per CU either way
template <int G>
struct KgShape {
  static constexpr u32 INBUF = G == 32 ? 12 : K1_INBUF;
  static constexpr bool COLD_IN_LDS = G != 32;  // (else: a gang's share of the windows must hold a GangCold while it builds)
};
constexpr u32 KG_RING_STRIDE = 36;     // LDS octets per lane of the token output ring (16 words + one dword of skew)
constexpr u32 KG_SUB_MIN = 1024;        // bits of bitstream per lane per round
constexpr u32 KG_SUB_MAX = 8192;
constexpr u64 KG_MULTI_BLOCK_BITS = 512u << 10;  // an item this long is taken to hold several blocks ...
constexpr u32 KG_BLOCK_GUESS_BITS = 192u << 10;  // ... of about this size (zlib: 16 K symbols of text)
constexpr u32 KG_OVL = 512;             // least run-up bits before a lane's sub-range (the host picks per gang width: 768 / 1024)

// lookup entries (u16).  bits 0-3: code length; 0 = not a symbol:
//     whole entry 0          unassigned pattern, or a long code without a second-level table -> exact step
//     otherwise              bits 4-6 = b, bits 7-15 = off: the symbol is at pool[off + next b stream bits]
//   lit/len:  bits 4-11 literal octet | (length base - 3);  bits 12-15: 0 literal, 8+X match with X extra
//             bits, 7 end of block, 6 symbol 286/287
//   distance: bits 4-8 distance symbol
template <u32 LPOOL, u32 DPOOL>
struct GangTablesT {  // per gang, in LDS
  u16 lfast[(1u << KG_TBL) + LPOOL];
  u16 dfast[(1u << KG_TBD) + DPOOL];  // while a header is parsed: octets 0-127 the code-length code's 7-bit
                                      // table, octets 128-447 the code lengths (the table is filled last)
  static_assert(((1u << KG_TBD) + DPOOL) * 2 >= 448, "dfast doubles as header scratch");
  static_assert(((1u << KG_TBL) + LPOOL) * 2 >= 1024, "lfast doubles as the gzip header's CRC table");
};
// The canonical lists of a gang's two codes: what the BUILD works on and, afterwards, only the exact step reads (a handful
// of times per lane and round: end of block, a code without a second-level table, the limit).  Round 4: gangs of 32 and 64
// build them in the LDS of their input windows — dead while a code is built — and park them in the item's scratch in
// memory (K1gParams::cold), so that the workgroup's LDS falls from 13.3 to 9.9 KB: sixteen workgroups per CU, four waves
// per SIMD.  Narrower gangs (four or eight sets of tables per workgroup: LDS-bound anyway) keep them in LDS.
struct GangCold {
  u16 lsym[288];            // lit/len symbols in canonical order
  u8 dsym[32];
  u32 llim[16];             // [0..14] left-aligned limits, [15] shortest code length
  u32 dlim[16];
  u16 ldlt[16];             // slot in canonical order = (code of length L) + dlt[L]  (mod 2^16)
  u16 ddlt[16];
};
constexpr u32 KG_COLD_STRIDE = 1024;  // octets of scratch per item for its GangCold
static_assert(sizeof(GangCold) == 800 && sizeof(GangCold) <= KG_COLD_STRIDE && sizeof(GangCold) % 4 == 0, "GangCold");
template <class GT>
TBZ_DEV u8* kg_lens(GT& gt) { return (u8*)gt.dfast + 128; }
enum { GM_HEADER = 0, GM_BUILD = 1, GM_BLOCK = 2, GM_DONE = 3 };
struct GangState {  // per gang, in LDS; owned by the leader
  u64 P;            // GM_BLOCK: bit position of the next token; GM_HEADER: of the next block header
  u64 T;            // token words committed so far
  u64 produced;     // octets those tokens produce
  u64 blk_pos, blk_prod, blk_tok;
  u64 fail_pos;
  i32 status;
  u32 mode, bfinal, deficit, tables, land, tr0, tr1, tr_have;
  u32 nruns, blk_runs;      // runs recorded so far / at the start of the current block
  RunRec run0;              // the item's first run (the others are in its run table)
  u32 hlit, hdist, fixed;   // GM_BUILD: alphabet sizes; fixed: 1 the lanes write the fixed code lengths first,
                            //   2 they copy the lengths K1h left in the item's scratch
  u32 rounds, valid_lanes;  // diagnostics: rounds run and lanes committed (efficiency = valid_lanes / (G*rounds))
  u32 cut;                  // 2: ran out of input inside a stored block's payload (SegResult.pad)
  u32 inl;                  // 1: a committed lane passed a block header inside its run (see Inl): the current block does
                            //   not start on a run boundary, so an overshoot cannot be rolled back to it (-> SEG_REDO)
  u32 noinline;             // 1: the next round decodes block by block (the round before was cut at a wrong assumption)
  u32 est;                  // expected bits of the current block, header included (0: no idea): the item's previous
                            //   block's.  A round is sized to what is left of the BLOCK, not of the item: the lanes
                            //   beyond an end-of-block code decode nothing that counts (measured on 256 KiB gzip members
                            //   of five blocks each: 17 of 64 lanes committed in a block's first round)
  u32 min_len;              // shortest code length of the current lit/len code | of the distance code << 8 (GangCold::llim[15], dlim[15])
  u32 ptry;                 // 1: the round before committed next to nothing (lanes do not fall into step: a PERIODIC bitstream —
                            //   a run of one repeated match, zeros in a file, config 5): the next round tries kg_periodic
};
template <int G, bool COLD_IN_LDS>
struct KgColdLds {
  GangCold cold[64 / G];
};
template <int G>
struct KgColdLds<G, false> {};
template <int G>
struct KgLds {
  static constexpr bool COLD_IN_LDS = KgShape<G>::COLD_IN_LDS;
  using GT = GangTablesT<KgPools<G>::L, KgPools<G>::D>;
  GT gt[64 / G];
  GangState gs[64 / G];
  u32 inbuf[KgShape<G>::INBUF][64];
  u8 tokring[64 * KG_RING_STRIDE];  // per lane: 16 token words on their way to memory (see TokOut)
  KgColdLds<G, COLD_IN_LDS> c;
#ifdef TBZ_EXP_LDSPAD
  u8 exp_pad[TBZ_EXP_LDSPAD];       // (occupancy experiment: profiles/README.md)
#endif
#ifdef TBZ_WAVE_TRACE
  u32 tr_cnt[4];
#endif
};

struct K1gParams {
  const u8* in_base;
  u16* tok;       // token pool: the word index of bit position x is (x >> half) & ~7 — lane g of a round writes its run
                  // from tok[slot(s_g)]
  RunRec* runs;   // run tables
  u32 half;       // 1: the pool holds one word per TWO input bits (a token of ordinary data takes far more; a lane whose
                  // region fills up ends its run early, and an item that does not fit is declined: SEG_REDO); 0: per bit
  u32 only_wide;  // 1 (gangs of 64 beside a narrow launch): decode the items longer than wide_bits and nothing else
  const Item* items;
  SegResult* res;
  const u64* markers;
  const u32* first_marker;  // [n_streams+1]
  const HdrRec* hdr;        // K1h's records (nullptr: none), and the code lengths they refer to
  const u8* hdr_lens;       //   … at hdr_lens[item * K1_SCRATCH ...]
  u32 n_markers;
  u32 n_items;
  u32 ovl;                  // run-up bits before a lane's sub-range (KG_OVL; wider gangs need longer chains of lanes
                            // in sync and take a longer run-up)
  u32 sub_min;              // least sub-range per lane (bits, multiple of 64): what the rounds after the first one run at
  u64 wide_bits;            // gangs narrower than 64 decline items longer than this (SEG_WIDE; 0: never)
  u64 resume_bit;           // ITEM_RESUME: where the token loop of the item's first block is entered
  u8* cold;                 // n_items * KG_COLD_STRIDE octets: where gangs of 32 / 64 keep their canonical lists (GangCold)
#ifdef TBZ_WAVE_TRACE
  u64* trace;               // experiment builds only: 8 words per workgroup (tools/exp/wave_trace.py)
#endif
};


struct __attribute__((packed, aligned(2))) U16x8 {  // eight token words at 2-octet alignment
  uint4 v;
};

// position the reader at `pos` with a freshly loaded window
TBZ_DEV void br_seek_fill(BitReader& b, u64 pos) {
  b.wi = (pos + b.bias) >> 5;
  br_refill(b);
  br_seek(b, pos);
}
// keep the words br_skip will want inside the window
TBZ_DEV void br_ensure(BitReader& b) {
  if (b.wi + 4 > b.bw + b.nw) br_refill(b);
}

TBZ_DEV u32 kg_lit_entry(u32 sym, u32 L) {
  u32 base, X;
  len_base_extra((sym - 257) & 31, base, X);
  u32 m = L | ((base - 3) << 4) | ((8 | X) << 12);
  return sym < 256 ? (L | (sym << 4)) : sym == 256 ? (L | (7u << 12)) : sym > 285 ? (L | (6u << 12)) : m;
}

// first-/second-level entry of a distance code: everything the hot loop needs, pre-chewed —
// bits 0-3 code length | 4-8 symbol | 9-12 extra-bit count | 13-14 mantissa m | 15 valid (symbol < 30), with
// distance - 1 = (m << extra-bit count) + extra bits  (RFC 1951 3.2.5: m = 2|(sym&1) from symbol 2 on)
TBZ_DEV u32 kg_dist_entry(u32 sym, u32 L) {
  const u32 DX = sym < 4 ? 0u : (sym >> 1) - 1;
  const u32 m = sym < 2 ? sym : (2u | (sym & 1));
  return L | (sym << 4) | (DX << 9) | (m << 13) | (sym < 30 ? 0x8000u : 0u);
}

// Canonical code of one alphabet built by the G lanes of a gang (same acceptance rules as build_canon:
// huffman-tree.lisp:112-122), plus its two-level lookup table.  EVERY lane of the wave calls this (it
// contains wave collectives); a gang that is not building passes n = 0 and touches nothing.
template <int G, u32 TB, u32 POOL, bool LIT, typename SymT>
TBZ_DEV i32 kg_build(const u8* lens, u32 n, SymT* sorted, u32* lim, u16* dlt, u16* fast, u32 g, u32 base) {
  const bool leader = g == 0;
  // 1. per-lane chunk of symbols: counts per code length, two 16-bit counters per word
  const u32 ch = (n + G - 1) / G;
  const u32 i0 = g * ch;
  const u32 i1 = i0 + ch < n ? i0 + ch : n;
  u32 own[8];
#pragma unroll
  for (int k = 0; k < 8; k++) own[k] = 0;
  for (u32 i = i0; i < i1; i++) {
    const u32 l = lens[i];
    const u32 inc = l ? 1u << ((l & 1) * 16) : 0u;
    const u32 w = l >> 1;
#pragma unroll
    for (int k = 0; k < 8; k++) own[k] += w == (u32)k ? inc : 0u;
  }
  // 2. gang prefix sums: symbols of each length in the chunks before mine, and the totals
  u32 inc_[8];
#pragma unroll
  for (int k = 0; k < 8; k++) inc_[k] = own[k];
#pragma unroll
  for (u32 d = 1; d < (u32)G; d <<= 1) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const u32 t = tbz_shfl_up(inc_[k], d);
      inc_[k] += g >= d ? t : 0u;
    }
  }
  u32 tot[8];
#pragma unroll
  for (int k = 0; k < 8; k++) tot[k] = tbz_shfl(inc_[k], (int)(base + G - 1));
  // 3. canonical parameters (every lane computes them; the leader publishes what the decoders read)
  u32 used = 0, code = 0, off = 0, prev = 0, min_len = 0;
  i32 left = 1, err = 0;
  u32 offp[8];
#pragma unroll
  for (int k = 0; k < 8; k++) offp[k] = 0;
#pragma unroll
  for (int L = 1; L < 16; L++) {
    const u32 c = (tot[L >> 1] >> ((L & 1) * 16)) & 0xffffu;
    left <<= 1;
    if ((i32)c > left && !err) err = E_OVERSUB;
    left -= (i32)c;
    used += c;
    if (c && !min_len) min_len = L;
    code = (code + prev) << 1;
    prev = c;
    offp[L >> 1] |= off << ((L & 1) * 16);
    const u32 limL = (code + c) << (16 - L);
    if (leader && n) {
      dlt[L] = (u16)(off - code);
      lim[L - 1] = limL;
    }
    off += c;
  }
  if (leader && n) lim[15] = min_len;
  if (!err && left > 0 && used > 1) err = E_INCOMPLETE;
  if (!err && used == 1 && min_len > 10) err = E_TREE_OVERFLOW;  // (as build_canon: huffman-tree.lisp:213-217)
  const bool ok = n != 0 && err == 0;
  // 4. canonical order: slot = first slot of the length + same-length symbols before this one
  u32 nxt[8];
#pragma unroll
  for (int k = 0; k < 8; k++) nxt[k] = offp[k] + inc_[k] - own[k];
  if (ok) {
    for (u32 i = i0; i < i1; i++) {
      const u32 l = lens[i];
      if (!l) continue;
      const u32 w = l >> 1, sh = (l & 1) * 16;
      u32 v = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) v = w == (u32)k ? nxt[k] : v;
#pragma unroll
      for (int k = 0; k < 8; k++) nxt[k] += w == (u32)k ? (1u << sh) : 0u;
      sorted[(v >> sh) & 0xffffu] = (SymT)i;
    }
  }
  tbz_sync();  // the limits are read back from LDS below (keeps fifteen registers free for the rest of the kernel)
  // 5. second-level sizes: a prefix whose codes are longer than TB bits gets 2^(longest - TB) pool entries.
  //    Lane g owns the left-aligned (MSB-first) prefixes [g*R, (g+1)*R); long prefixes are the ones at or
  //    above the first value no code of <= TB bits reaches.
  constexpr u32 R = (1u << TB) / G;
  constexpr u32 SH = 16 - TB;
  const u32 r0 = g * R;
  u32 need = 0;
  if (ok) {
#pragma nounroll
    for (u32 j = g; j < POOL; j += G) fast[(1u << TB) + j] = 0;
#pragma nounroll
    for (u32 t = 0; t < R; t++) {
      const u32 r16 = (r0 + t) << SH;
      if (r16 < lim[TB - 1]) continue;
      const u32 last = r16 | ((1u << SH) - 1);
      u32 Lm = TB + 1;
#pragma unroll
      for (u32 q = TB; q < 15; q++) Lm += last >= lim[q] ? 1u : 0u;
      if (Lm <= 15) need += 1u << (Lm - TB);
    }
  }
  u32 pin = need;
#pragma unroll
  for (u32 d = 1; d < (u32)G; d <<= 1) {
    const u32 t = tbz_shfl_up(pin, d);
    pin += g >= d ? t : 0u;
  }
  const u32 ptot = tbz_shfl(pin, (int)(base + G - 1));
  const bool two = ptot <= POOL;  // else: no second level, long codes go through the exact step
  tbz_sync();
  // 6. first level: symbols are monotone in the prefix, so one compare-count decode serves a run of entries
  if (ok) {
    u32 r = r0, end_r = r, entry = 0, poff = pin - need;
#pragma nounroll
    for (u32 t = 0; t < R; t++, r++) {
      if (r >= end_r) {
        const u32 r16 = r << SH;
        u32 L = 1;
#pragma unroll
        for (int k = 0; k < 15; k++) L += r16 >= lim[k] ? 1u : 0u;
        if (L <= TB) {
          const u32 slot = ((r16 >> (16 - L)) + dlt[L]) & 0xffffu;
          const u32 sym = sorted[slot < n ? slot : 0];
          entry = LIT ? kg_lit_entry(sym, L) : kg_dist_entry(sym, L);
          end_r = ((r >> (TB - L)) + 1) << (TB - L);
        } else {
          const u32 last = r16 | ((1u << SH) - 1);
          u32 Lm = TB + 1;
#pragma unroll
          for (u32 q = TB; q < 15; q++) Lm += last >= lim[q] ? 1u : 0u;
          entry = 0;
          if (L <= 15 && Lm <= 15) {
            if (two) entry = ((Lm - TB) << 4) | (poff << 7);
            poff += 1u << (Lm - TB);
          }
          end_r = r + 1;
        }
      }
      fast[tbz_brev32(r) >> (32 - TB)] = (u16)entry;
    }
  }
  tbz_sync();
  // 7. second level, spread over the lanes by canonical slot
  if (ok && two) {
    const u32 kfirst = (offp[(TB + 1) >> 1] >> (((TB + 1) & 1) * 16)) & 0xffffu;  // symbols with codes <= TB bits
    for (u32 k = kfirst + g; k < used; k += G) {
      u32 L = TB + 1;
#pragma unroll
      for (u32 q = TB + 2; q < 16; q++) L += k >= ((offp[q >> 1] >> ((q & 1) * 16)) & 0xffffu) ? 1u : 0u;
      const u32 cd = (k - dlt[L]) & 0xffffu;
      const u32 e1 = fast[tbz_brev32(cd >> (L - TB)) >> (32 - TB)];
      if (e1 == 0) continue;
      const u32 b = (e1 >> 4) & 7, po = e1 >> 7, xl = L - TB;
      const u32 j0 = tbz_brev32(cd & ((1u << xl) - 1)) >> (32 - xl);
      const u32 sym = sorted[k];
      const u32 entry = LIT ? kg_lit_entry(sym, L) : kg_dist_entry(sym, L);
      for (u32 j = j0; j < (1u << b); j += 1u << xl) fast[(1u << TB) + po + j] = (u16)entry;
    }
  }
  return n ? err : 0;
}

#define KG_CHECK(p0)                 \
  do {                               \
    if (st.br.pos > st.end_bit) {    \
      st.fail_pos = (p0);            \
      return SEG_UNDERRUN;           \
    }                                \
    if (st.br.pos > st.limit_bit) {  \
      st.fail_pos = (p0);            \
      return SEG_OVERSHOOT;          \
    }                                \
  } while (0)

// leader: :dynamic-huffman-block … :dht-len-table-data (deflate.lisp:577-669): leaves the code lengths
// in kg_lens(gt) and the alphabet sizes in gs.hlit / gs.hdist
template <class GT>
TBZ_DEV i32 kg_dynamic_header(GT& gt, GangState& gs, K1State& st) {
  const u64 p0 = st.br.pos;
  u32 pk = br_peek(st.br);
  const u32 hlit = (pk & 31) + 257, hdist = ((pk >> 5) & 31) + 1, hclen = ((pk >> 10) & 15) + 4;
  br_skip(st.br, 14);
  KG_CHECK(p0);
  u8* lens = kg_lens(gt);
  for (u32 i = 0; i < 19; i++) lens[i] = 0;
  for (u32 i = 0; i < hclen; i++) {
    const u32 v = br_peek(st.br) & 7;
    br_skip(st.br, 3);
    lens[c_cl_order[i]] = (u8)v;
  }
  KG_CHECK(p0);
  // the code-length code: canonical codes of <= 7 bits -> 128-entry table (len | sym << 3; 0 = unassigned)
  u8* cl = (u8*)gt.dfast;
  u16* cnt = gt.lfast;        // scratch: the lit/len table is filled after the header
  u16* nextc = gt.lfast + 8;
  for (int L = 0; L < 8; L++) cnt[L] = 0;
  for (u32 i = 0; i < 19; i++) cnt[lens[i]] += 1;
  u32 used = 0, code = 0, prev = 0, cl_min = 0;
  i32 left = 1, err = 0;
  for (int L = 1; L < 8; L++) {
    const u32 c = cnt[L];
    left <<= 1;
    if ((i32)c > left && !err) err = E_OVERSUB;
    left -= (i32)c;
    used += c;
    if (c && !cl_min) cl_min = L;
    code = (code + prev) << 1;
    prev = c;
    nextc[L] = (u16)code;
  }
  if (!err && left > 0 && used > 1) err = E_INCOMPLETE;
  if (err) return err;
  for (u32 j = 0; j < 128; j += 4) *(u32*)(cl + j) = 0;
  for (u32 i = 0; i < 19; i++) {
    const u32 l = lens[i];
    if (!l) continue;
    const u32 cd = nextc[l];
    nextc[l] = (u16)(cd + 1);
    const u32 rev = tbz_brev32(cd) >> (32 - l);
    for (u32 j = rev; j < 128; j += 1u << l) cl[j] = (u8)(l | (i << 3));
  }
  const u32 n = hlit + hdist;
  u32 i = 0, last = 0xff;
  {
    // Fast pass: the same decode on 32-bit window state (as the token loop), repeats stored eight at a
    // time, no per-symbol position checks.  Anything unusual — unassigned pattern, a repeat error,
    // running past the end / the limit — abandons it, and the exact loop below redoes the header.
    const BitReader save = st.br;
    const u32 lane = tbz_lane();
    const u64 lim64 = st.end_bit < st.limit_bit ? st.end_bit : st.limit_bit;
    BitReader& B = st.br;
    bool slow = false;
    while (i < n && !slow) {
      br_refill(B);
      u32 lo = B.lo, hi = B.hi, nx = B.nx, o = B.o, k = 3, rel = 0;
      i32 rem = lim64 <= B.pos ? 0 : ((lim64 - B.pos) > 0x7fffff00ull ? 0x7fffff00 : (i32)(lim64 - B.pos));
      const u32* wp = &B.buf[3][lane];
      while (i < n && k + 1 <= B.nw) {
        const u32 x1 = wp[0];
        const u32 pk = tbz_alignbit(hi, lo, o);
        const u32 e = cl[pk & 127];
        const u32 L = e & 7, sym = e >> 3;
        const u32 xb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        const u32 x = tbz_bfe(pk, L, xb), nb = L + xb;
        if (L == 0 || rem < (i32)nb) {
          slow = true;
          break;
        }
        if (sym < 16) {
          lens[i++] = (u8)sym;
          last = sym;
        } else {
          const u32 rep = (sym == 18 ? 11u : 3u) + x;
          const u32 val = sym == 16 ? last : 0u;
          if ((sym == 16 && last >= 16) || i + rep > n) {
            slow = true;
            break;
          }
          const u64 v8 = (u64)val * 0x0101010101010101ull;
          for (u32 q = 0; q < rep; q += 8) k2_st64(lens + i + q, v8);  // spills <= 7 octets into entries not yet written
          i += rep;
          last = val;
        }
        rem -= (i32)nb;
        rel += nb;
        o += nb;
        const bool adv = o >= 32;
        o &= 31;
        lo = adv ? hi : lo;
        hi = adv ? nx : hi;
        nx = adv ? x1 : nx;
        k += adv ? 1u : 0u;
        wp += adv ? 64 : 0;
      }
      B.pos += rel;
      B.wi += k - 3;
      B.lo = lo;
      B.hi = hi;
      B.nx = nx;
      B.o = o;
    }
    if (slow) {
      st.br = save;
      br_seek_fill(st.br, save.pos);  // the LDS window has moved on since `save` was taken
      i = 0;
      last = 0xff;
    }
  }
  while (i < n) {
    br_ensure(st.br);
    const u64 ps = st.br.pos;
    pk = br_peek(st.br);
    const u32 e = cl[pk & 127];
    const u32 L = e & 7, sym = e >> 3;
    if (L == 0) {  // unassigned pattern: error unless the input ends inside the root index
      if (st.br.pos + cl_min > st.end_bit) {
        st.fail_pos = ps;
        return SEG_UNDERRUN;
      }
      return E_INVALID_CODE;
    }
    const u32 xb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
    const u32 x = tbz_bfe(pk, L, xb);
    br_skip(st.br, L + xb);
    KG_CHECK(ps);
    if (sym < 16) {
      lens[i++] = (u8)sym;
      last = sym;
    } else {
      u32 rep, val;
      if (sym == 16) {
        if (last >= 16) return E_REPEAT_NO_PREV;
        rep = 3 + x;
        val = last;
      } else {
        rep = (sym == 17 ? 3 : 11) + x;
        val = 0;
        last = 0;
      }
      if (i + rep > n) return E_REPEAT_OVERRUN;
      for (u32 k = 0; k < rep; k++) lens[i + k] = (u8)val;
      i += rep;
    }
  }
  gs.hlit = hlit;
  gs.hdist = hdist;
  return 0;
}
#undef KG_CHECK

// what one lane reports for one round
enum { RF_STOP = 0, RF_EOB, RF_LIMIT, RF_CODE_LIT, RF_CODE_DIST, RF_SYM, RF_JUNK };
struct RoundOut {
  u64 c;     // bit position where the lane started recording (~0: never did)
  u64 e;     // RF_STOP: start of the first token at/after `stop`; RF_EOB: bit after the end-of-block code;
             // failures: start of the failing token
  u64 aux;   // failures: bit position reached inside the failing token
  u32 n;     // token words staged
  u32 out;   // octets they produce
  i32 mdef;  // max over recorded matches of (distance - octets this lane produced before the match)
  u32 flag;
  // fixed-Huffman blocks that follow each other are decoded THROUGH (see Inl): while recording, the lane passed
  u64 hdr;      //   … its last block header at this bit position (valid when nhdr != 0)
  u32 nhdr;     //   … this many block headers
  u32 assumed;  //   … an end-of-block code without knowing whether that block was the final one (it took it not to be)
  i32 bf_end;   // BFINAL of the block the lane was in when it stopped, -1 = the block it started in (no header passed)
#ifdef TBZ_WAVE_TRACE
  u32 li;
#endif
};
// Decoding through block boundaries inside a lane's sub-range.  With the fixed code loaded (deflate.lisp:518-528 ->
// ht-constants.lisp:9-32) the tables do not change from block to block, so "end-of-block, BFINAL, BTYPE=1" is consumed
// like a token and the lane goes on; anything else after an end-of-block code stops the lane as before.  A lane that
// began inside a block does not know that block's BFINAL: it assumes 0 and says so; the commit step, which knows
// BFINAL lane by lane along the chain, cuts the round where the assumption was wrong.
struct Inl {
  bool on;
  i32 cur_bf;  // BFINAL of the block the reader is in: -1 unknown
};
// A lane's token output.  Storing every token straight to memory is a 2- or 4-octet store per lane into 64
// different cache lines per instruction, and the lines leave L2 partly written (measured: 4.7 GB of write
// traffic for 1.3 GB of tokens, 0.75 ms of the kernel).  Instead the words go through a 16-word ring in LDS
// (stride of 9 dwords per lane: conflict-free) and leave as whole 16-octet pieces.
struct TokOut {
  u8* ring;    // this lane's 32 octets of LDS
  u16* stage;  // where the run goes in the token pool (16-octet aligned)
  u32 n;       // words produced
  u32 nf;      // words already stored (multiple of 8)
#ifdef TBZ_WAVE_TRACE
  u32 li;    // this lane's iterations
  u32* cnt;  // LDS: wave trips of the token loop, phases
#endif
};
TBZ_DEV void tok_put(TokOut& t, u32 w) { *(u16*)(t.ring + ((t.n & 15) << 1)) = (u16)w; }
TBZ_DEV void tok_put2(TokOut& t, u32 w) {  // words n and n+1 from the halves of w
  *(u16*)(t.ring + ((t.n & 15) << 1)) = (u16)w;
  *(u16*)(t.ring + (((t.n + 1) & 15) << 1)) = (u16)(w >> 16);
}
TBZ_DEV void tok_flush_piece(TokOut& t) {  // the oldest 8 words
#ifdef TBZ_WAVE_TRACE
  if (tbz_exp_flags & 1) {
    t.nf += 8;
    return;
  }
  if (tbz_exp_flags & 2) {
    *(uint4*)(t.stage + (t.nf & 63)) = *(const uint4*)(t.ring + ((t.nf & 15) << 1));
    t.nf += 8;
    return;
  }
#endif
  *(uint4*)(t.stage + t.nf) = *(const uint4*)(t.ring + ((t.nf & 15) << 1));
  t.nf += 8;
}
struct __attribute__((packed, aligned(2))) U32at2 {  // two token words stored at once
  u32 v;
};

// The hot loop.  Decodes tokens from the reader's position until a token starts at or after `target`
// (returns 0), or the next token is anything but a plain literal / valid match inside the limit
// (returns 1 with the reader AT that token; kg_exact_step sorts it out).  Phases as in k1_decode_block: the lane's
// LDS window is reloaded, then at most K1_PHASE trips run out of LDS with no global load in between (vmcnt is one
// in-order counter per wave).
//
// Round 4: the loop is priced in VECTOR instructions — tools/issue_roof.hip: a gfx950 SIMD retires ~0.57 integer VALU
// wave-instructions per ns chip-wide whatever the occupancy (the clock gives way under load), scalar and LDS
// instructions ride along nearly free, and this kernel sat at 0.38.  So the trip keeps NO shifting register window
// (three words + two prefetched + a three-way select per advance: 11 VALU): the position is ONE register `p`, bits from
// the window's first word, and every trip reads its three words straight from the lane's LDS column (conflict-free:
// word k of lane l is bank l); target and limit are kept in the same coordinates (no rel / rem counters); the distance
// code's bits come from one funnel shift of the 64 bits at p (`pk2:pk` >> n1, n1 <= 20) instead of two shifts and a select.
template <bool REC, class GT>
TBZ_DEV u32 kg_span(const GT& gt, BitReader& B, u64 target, u64 lim64, TokOut& to, u32 cap, u32& out_,
                    i32& mdef_) {
  const u32 lane = tbz_lane();
  u32 out = out_;
  u32& n = to.n;
  i32 mdef = mdef_;
  u32 ret;
  const u8* wcol = (const u8*)&B.buf[0][lane];  // word k of this lane's window: wcol + 256 * k
  for (;;) {
    br_refill(B);
    const u32 o0 = B.o;
    const u32 remb = lim64 <= B.pos ? 0u : ((lim64 - B.pos) > 0x7fffff00ull ? 0x7fffff00u : (u32)(lim64 - B.pos));
    u32 tgtb = target <= B.pos ? 0u : ((target - B.pos) > 0x7fffff00ull ? 0x7fffff00u : (u32)(target - B.pos));
    if (REC && n + 2 * KG_PHASE > cap) tgtb = 0;  // staging region nearly full: end the lane's run here
    const u32 limp = remb + o0, tgtp = tgtb + o0;  // (window coordinates: bit 0 = bit 0 of the window's first word)
    // a trip reads the words (p >> 5) .. (p >> 5) + 2 of the window
    const u32 wend = (B.nw - 2) * 32;
    const u32 stop_p = tgtp < wend ? tgtp : wend;
    u32 p = o0, it = 0;
    bool bad = false;
    // NOTE: conditions are combined with & and | on purpose — && / || / ?: on side-effect-free terms
    // become exec-mask branches here, and every branch costs the whole wave scalar work
    bool go = p < stop_p;
#ifdef TBZ_WAVE_TRACE
    if (lane == (u32)__builtin_ctzll(tbz_ballot(true))) atomicAdd(&to.cnt[1], 1u);
#endif
    while (go) {
#ifdef TBZ_WAVE_TRACE
      if (lane == (u32)__builtin_ctzll(tbz_ballot(true))) atomicAdd(&to.cnt[0], 1u);
      to.li++;
#endif
      const u32* w = (const u32*)(wcol + ((p >> 5) << 8));
      const u32 w0 = w[0], w1 = w[64], w2 = w[128];
      const u32 pk = tbz_alignbit(w1, w0, p & 31), pk2 = tbz_alignbit(w2, w1, p & 31);  // bits p .. p+63
      u32 e = gt.lfast[pk & ((1u << KG_TBL) - 1)];
      if (((e & 15) == 0) & (e != 0)) e = gt.lfast[(1u << KG_TBL) + (e >> 7) + tbz_bfe(pk, KG_TBL, (e >> 4) & 7)];
      const u32 L = e & 15;
      const bool isM = e >= 0x8000u;
      const u32 X = tbz_bfe(e, 12, 3);  // literals carry 0 here; end-of-block / invalid entries are not `good` below
      const u32 n1 = L + X;             // <= 20
      const u32 pd = tbz_alignbit(pk2, pk, n1);  // the 32 bits after the length code and its extra bits
      // both speculative lookups go out together: the distance code of a match, and the code after a literal
      const u32 e2 = gt.lfast[tbz_bfe(pk, L, KG_TBL)];
      u32 ed = gt.dfast[pd & ((1u << KG_TBD) - 1)];
      if (isM & ((ed & 15) == 0) & (ed != 0)) ed = gt.dfast[(1u << KG_TBD) + (ed >> 7) + tbz_bfe(pd, KG_TBD, (ed >> 4) & 7)];
      const u32 DL = ed & 15, DX = tbz_bfe(ed, 9, 4);  // kg_dist_entry
      const u32 pe = p + (isM ? n1 + DL + DX : L);     // where the token ends
      const bool okm = ed >= 0x8000u, okl = e < 0x1000u;
      // (a token that is not `good` consumes nothing, records nothing and ends the lane's loop — by predication, not by
      // a break: every exit from a divergent loop costs the whole wave exec-mask bookkeeping on the scalar unit)
      const bool good = (L != 0) & (isM ? okm : okl) & (pe <= limp);
      bad = !good;
      // a second literal rides along when the code after a literal is a first-level literal too (it must
      // start before the target and end inside the limit): literal-dense sub-ranges are the slow lanes
      const u32 L2 = e2 & 15;
      const bool pair = good & !isM & (L2 != 0) & (e2 < 0x1000u) & (pe < tgtp) & (pe + L2 <= limp);
      p = good ? pe + (pair ? L2 : 0u) : p;
      if (REC) {
        const u32 lenx = ((e >> 4) & 0xffu) + tbz_bfe(pk, L, X);           // literal octet, or match length - 3
        const u32 dm1 = (tbz_bfe(ed, 13, 2) << DX) + tbz_bfe(pd, DL, DX);  // distance - 1
        // literal: 0x00bb (the high half is the second literal of a pair, or overwritten by the next token);
        // match: head | payload << 16
        tok_put2(to, isM ? (TOK_MATCH | lenx | (dm1 << 16)) : (lenx | (((e2 >> 4) & 0xffu) << 16)));
        const i32 d = (i32)dm1 + 1 - (i32)out;
        mdef = (good & isM & (d > mdef)) ? d : mdef;
        const u32 cnt = good ? ((isM | pair) ? 2u : 1u) : 0u;
        n += cnt;
        out += (good & isM) ? lenx + 3 : cnt;
      }
      if (REC && (it & 1)) {  // every other token: a whole 16-octet piece leaves the ring (at most 4 words came in)
        if (to.n - to.nf >= 8) tok_flush_piece(to);
      }
      it++;
      go = good & (it < KG_PHASE) & (p < stop_p);
    }
    // the reader's POSITION, at p.  Its three words of lookahead (lo / hi / nx) are left stale: whoever reads next —
    // the next phase, kg_exact_step, a header parse — reloads the window and seeks first (br_refill / br_seek_fill), and
    // fetching them here would be up to three words from beyond the window, i.e. a memory round trip per phase
    B.pos += p - o0;
    B.wi += p >> 5;
    B.o = p & 31;
    // (a span of ONE token never reaches the flush above: blocks of a single literal, decoded through)
    if (REC && to.n - to.nf >= 8) tok_flush_piece(to);
    if (bad) { ret = 1; break; }
    if (p >= tgtp) { ret = 0; break; }
  }
  out_ = out;
  mdef_ = mdef;
  return ret;
}

// full compare-count decode out of the gang's canonical lists (cold path)
TBZ_DEV u32 kg_canon_lds(u32 pk, const u32* lim, const u16* dlt, u32 cap, u32& slot) {
  const u32 r16 = tbz_brev32(pk) >> 16;
  u32 L = 1;
  for (int k = 0; k < 15; k++) L += r16 >= tbz_ld_agent(lim + k) ? 1u : 0u;  // (the lists may live in memory: GangCold)
  u32 sl = ((r16 >> (16 - (L & 15))) + tbz_ld_agent(dlt + (L & 15))) & 0xffffu;
  slot = sl < cap ? sl : 0;
  return L;
}

// The exact step: decode ONE token at the reader's position the long way (no lookup tables), with the
// reference's failure rules.  Returns 0 if it was a literal or match inside the limit (consumed, and
// recorded when `rec`); otherwise fills ro.flag / ro.e / ro.aux and returns 1.
TBZ_DEV u32 kg_exact_step(const GangCold& gc, BitReader& B, u64 lim64, bool rec, TokOut& to, u32& out, i32& mdef,
                          RoundOut& ro, Inl& il) {
  const u64 p0 = B.pos;
  br_seek_fill(B, p0);
  const u32 pk = br_peek(B);
  u32 slot;
  const u32 L = kg_canon_lds(pk, gc.llim, gc.ldlt, 288, slot);
  ro.e = p0;
  if (L > 15) {
    ro.flag = RF_CODE_LIT;
    ro.aux = p0;
    return 1;
  }
  const u32 sym = tbz_ld_agent(gc.lsym + slot);
  if (sym <= 256 || sym > 285) {
    br_skip(B, L);
    ro.aux = B.pos;
    if (B.pos > lim64) {
      ro.flag = RF_LIMIT;
      return 1;
    }
    if (sym == 256) {
      if (il.on && il.cur_bf != 1 && B.pos + 3 <= lim64) {
        const u32 h = br_peek(B);
        if (((h >> 1) & 3) == 1) {  // another fixed-Huffman block: through it
          if (rec) {
            if (il.cur_bf < 0) ro.assumed = 1;
            ro.hdr = B.pos;
            ro.nhdr += 1;
            ro.bf_end = (i32)(h & 1);
          }
          il.cur_bf = (i32)(h & 1);
          br_skip(B, 3);
          return 0;
        }
      }
      ro.flag = RF_EOB;
      ro.e = B.pos;
      return 1;
    }
    if (sym > 285) {  // 286/287 are coded but may not be used (huffman-tree.lisp:176-177)
      ro.flag = RF_SYM;
      return 1;
    }
    if (rec) {
      tok_put(to, sym);
      to.n += 1;
      out += 1;
      if (to.n - to.nf >= 8) tok_flush_piece(to);
    }
    return 0;
  }
  u32 base, X;
  len_base_extra(sym - 257, base, X);
  const u32 len = base + tbz_bfe(pk, L, X);
  br_skip(B, L + X);
  const u32 pd = br_peek(B);
  const u32 DL = kg_canon_lds(pd, gc.dlim, gc.ddlt, 32, slot);
  ro.aux = B.pos;
  if (DL > 15) {
    ro.flag = RF_CODE_DIST;
    return 1;
  }
  const u32 ds = tbz_ld_agent(gc.dsym + slot);
  if (ds > 29) {  // 30/31 (huffman-tree.lisp:172-175)
    br_skip(B, DL);
    ro.aux = B.pos;
    ro.flag = B.pos > lim64 ? RF_LIMIT : RF_SYM;
    return 1;
  }
  u32 dbase, DX;
  dist_base_extra(ds, dbase, DX);
  const u32 dist = dbase + tbz_bfe(pd, DL, DX);
  br_skip(B, DL + DX);
  ro.aux = B.pos;
  if (B.pos > lim64) {
    ro.flag = RF_LIMIT;
    return 1;
  }
  if (rec) {
    const i32 d = (i32)dist - (i32)out;
    mdef = d > mdef ? d : mdef;
    tok_put2(to, (TOK_MATCH | (len - 3)) | ((dist - 1) << 16));
    to.n += 2;
    out += len;
    if (to.n - to.nf >= 8) tok_flush_piece(to);
  }
  return 0;
}

// One lane's share of a round: decode from `start`; tokens that start before rec_from are the run-up
// (not recorded), the ones from there to the first token start >= stop are staged.
template <class GT>
TBZ_DEV void kg_lane_round(const GT& gt, const GangCold& gc, BitReader& B, u64 start, u64 rec_from, u64 stop, u64 lim64,
                           u16* stage, u8* ring, u32 cap, RoundOut& ro, Inl il) {
  TokOut to;
  to.ring = ring;
  to.stage = stage;
  to.n = to.nf = 0;
#ifdef TBZ_WAVE_TRACE
  to.li = 0;
  to.cnt = (u32*)(ring - tbz_lane() * KG_RING_STRIDE + 64 * KG_RING_STRIDE);
#endif
  u32 out = 0;
  i32 mdef = -(1 << 30);
  br_seek_fill(B, start);
  bool junk = false;
  while (B.pos < rec_from) {  // run-up
    if (kg_span<false>(gt, B, rec_from, lim64, to, cap, out, mdef) == 0) break;
    const u64 q = B.pos;  // (the reader is AT the token the fast loop would not take)
    if (kg_exact_step(gc, B, lim64, false, to, out, mdef, ro, il)) {
      // An invalid code or an end-of-block code met during the run-up says the lane is not on the true token sequence
      // (or that the block ends before its sub-range: nothing of it will count then).  Giving up costs the round its
      // chain; starting over ONE BIT FURTHER ON is a new draw.  Measured on 32 KiB of random octets as fixed-Huffman
      // literals (codes of 8 and 9 bits: config 5's 294 Kbit block): 27 % of the starts die on a seven-zero end-of-block
      // or an unused distance code, 73 % of the lanes were in step after 512 bits; 96.5 % with the restart.  Whatever
      // the lane does here, it counts only if it starts recording exactly where its predecessor stops.
      if (ro.flag == RF_LIMIT || q + 1 >= rec_from) {
        junk = true;
        break;
      }
      br_seek_fill(B, q + 1);
      il.cur_bf = -1;
    }
  }
  ro.c = ~0ull;
  ro.n = 0;
  ro.out = 0;
  ro.mdef = mdef;
#ifdef TBZ_WAVE_TRACE
  ro.li = to.li;
#endif
  if (junk) {
    ro.flag = RF_JUNK;
    return;
  }
  ro.c = B.pos;
  for (;;) {
    if (kg_span<true>(gt, B, stop, lim64, to, cap, out, mdef) == 0) {
      ro.flag = RF_STOP;
      ro.e = B.pos;
      ro.aux = B.pos;
      break;
    }
    if (kg_exact_step(gc, B, lim64, true, to, out, mdef, ro, il)) break;
  }
  // the run is stored in whole 8-word granules: pad with no-ops and let the last pieces out
  ro.n = to.n;
  const u32 n8 = (to.n + 7) >> 3;
  for (u32 k = to.n; k < n8 * 8; k++) *(u16*)(to.ring + ((k & 15) << 1)) = (u16)TOK_NOP;
  while (to.nf < n8 * 8) tok_flush_piece(to);
  ro.out = out;
  ro.mdef = mdef;
#ifdef TBZ_WAVE_TRACE
  ro.li = to.li;
#endif
}

// ---- periodic bitstreams.  Speculative lanes fall into step because Huffman codes self-synchronise — unless the bits
// repeat: a shifted parse of a periodic stream is itself periodic and never meets the true one (a run of ONE repeated
// match: 258 zeros after 258 zeros, the commonest thing in sparse files; config 5 is made of it).  But there the true
// parse is known without decoding: if the token at P is T bits long and the raw bits from P to x are T-periodic, the
// decoder is at a token start at every P + kT up to x (same bits, same state: same token).  kg_token_bits: length of
// the plain literal / valid match at `pos`, 0 for anything else; kg_periodic: bits[x] == bits[x + T] over [x0, x1).
template <class GT>
TBZ_DEV u32 kg_token_bits(const GT& gt, BitReader& B, u64 pos, u64 lim64) {
  br_seek_fill(B, pos);
  const u32 pk = br_peek(B);
  u32 e = gt.lfast[pk & ((1u << KG_TBL) - 1)];
  if (((e & 15) == 0) & (e != 0)) e = gt.lfast[(1u << KG_TBL) + (e >> 7) + tbz_bfe(pk, KG_TBL, (e >> 4) & 7)];
  const u32 L = e & 15;
  if (L == 0) return 0;
  if (e < 0x1000u) return pos + L <= lim64 ? L : 0u;  // a literal
  if (e < 0x8000u) return 0;                          // end of block, 286/287
  const u32 X = tbz_bfe(e, 12, 3);
  br_skip(B, L + X);
  const u32 pd = br_peek(B);
  u32 ed = gt.dfast[pd & ((1u << KG_TBD) - 1)];
  if (((ed & 15) == 0) & (ed != 0)) ed = gt.dfast[(1u << KG_TBD) + (ed >> 7) + tbz_bfe(pd, KG_TBD, (ed >> 4) & 7)];
  if (ed < 0x8000u) return 0;
  const u32 T = L + X + (ed & 15) + tbz_bfe(ed, 9, 4);
  return pos + T <= lim64 ? T : 0u;
}
TBZ_DEV u32 kg_bits32(const BitReader& b, u64 pos) {
  const u64 a = pos + b.bias, i = a >> 5;
  return tbz_alignbit(br_word_global(b, i + 1), br_word_global(b, i), (u32)(a & 31));
}
TBZ_DEV bool kg_periodic(const BitReader& b, u64 x0, u64 x1, u32 T, u64 lim64) {
  if (x1 + T + 32 > lim64) return false;
  u32 diff = 0;
  for (u64 x = x0; x < x1; x += 32) diff |= kg_bits32(b, x) ^ kg_bits32(b, x + T);
  return diff == 0;
}

// run-table slots an item may use once it has consumed the bitstream up to `upto`: the table is
// position-addressed, so it must not grow into the slots of whatever starts after it
// where an item's tokens and run table live: in the launch's pools by position, or in a region of its own
struct ItemPool {
  u16* tok;      // token base: the 8-word granule of the start's slot (fix-up items start mid-octet)
  RunRec* runs;  // run table (entry 0 unused: GangState::run0)
  u32 half;      // log2 of the input bits per token word
  u64 slot0;     // word index of the item's start; a bit position x lives at tok[((x >> half) & ~7) - slot0]
};
TBZ_DEV ItemPool kg_item_pool(const Item& it, const K1gParams& P) {
  ItemPool ip;
  const bool own = (it.flags & ITEM_EXPLICIT) != 0;
  ip.half = own ? 0u : P.half;
  ip.slot0 = (it.start_bit >> ip.half) & ~7ull;
  ip.tok = own ? (u16*)it.tok : P.tok + ip.slot0;
  ip.runs = own ? (RunRec*)it.runs : P.runs + (it.start_bit >> RUN_SHIFT);
  return ip;
}
TBZ_DEV u32 kg_run_slots(const Item& it, u64 upto) {
  const u64 s = (upto - it.start_bit) >> RUN_SHIFT;
  return s < 1 ? 1u : (s > 0x7fffffffull ? 0x7fffffffu : (u32)s);
}

// leader: what follows a block (deflate.lisp:719-722 + the container trailers + landing rules)
TBZ_DEV void kg_block_end(GangState& gs, K1State& st, const Item& it, const K1gParams& P, u32 fmt, bool fixup) {
  if (gs.bfinal) {
    gs.status = SEG_FINAL;
    br_seek_fill(st.br, gs.P);
    br_skip(st.br, (u32)((0 - st.br.pos) & 7));
    if (fmt == 1) {
      if (st.br.pos + 32 <= st.end_bit) {
        u32 v = br_peek(st.br);
        br_skip(st.br, 32);
        gs.tr0 = (v >> 24) | ((v >> 8) & 0xff00) | ((v << 8) & 0xff0000) | (v << 24);
        gs.tr_have = 2;
      }
    } else if (fmt == 2) {
      if (st.br.pos + 32 <= st.end_bit) {
        gs.tr0 = br_peek(st.br);
        br_skip(st.br, 32);
        gs.tr_have = 1;
        if (st.br.pos + 32 <= st.end_bit) {
          gs.tr1 = br_peek(st.br);
          br_skip(st.br, 32);
          gs.tr_have = 2;
        }
      }
    } else {
      gs.tr_have = 2;
    }
    gs.P = st.br.pos;
    gs.mode = GM_DONE;
    return;
  }
  if (!fixup) {
    if (gs.P == st.limit_bit) {
      gs.status = SEG_LANDED;
      gs.mode = GM_DONE;
      return;
    }
  } else {
    u64 b = gs.P;
    u32 lo = P.first_marker[it.stream];
    const u32 hi0 = P.first_marker[it.stream + 1];
    u32 hi = hi0;
    while (lo < hi) {
      u32 mid = (lo + hi) >> 1;
      if (P.markers[mid] < b) lo = mid + 1; else hi = mid;
    }
    if (lo < hi0 && P.markers[lo] == b) {
      gs.land = lo;
      gs.status = SEG_LANDED;
      gs.mode = GM_DONE;
      return;
    }
  }
  gs.mode = GM_HEADER;
}

// leader: block header at gs.P (deflate.lisp:518-573); stored blocks are handled completely here,
// Huffman blocks leave the gang in GM_BUILD (or GM_BLOCK when the fixed code is already loaded)
template <class GT>
TBZ_DEV void kg_leader_header(GT& gt, GangState& gs, K1State& st, const Item& it, const K1gParams& P,
                              u16* tok0, u32 fmt, bool fixup, u32 idx) {
  br_seek_fill(st.br, gs.P);
  gs.blk_pos = gs.P;
  gs.blk_prod = gs.produced;
  gs.blk_tok = gs.T;
  gs.blk_runs = gs.nruns;
  gs.inl = 0;
  u32 pk = br_peek(st.br);
  br_skip(st.br, 3);
  if (st.br.pos > st.end_bit) { gs.fail_pos = gs.blk_pos; gs.status = SEG_UNDERRUN; gs.mode = GM_DONE; return; }
  if (st.br.pos > st.limit_bit) { gs.status = SEG_OVERSHOOT; gs.mode = GM_DONE; return; }
  gs.bfinal = pk & 1;
  const u32 btype = (pk >> 1) & 3;
  if (btype == 0) {
    br_skip(st.br, (u32)((0 - st.br.pos) & 7));
    const u64 ph = st.br.pos;
    u32 ln = br_peek(st.br);
    br_skip(st.br, 32);
    if (st.br.pos > st.end_bit) { gs.fail_pos = ph; gs.status = SEG_UNDERRUN; gs.mode = GM_DONE; return; }
    u32 LEN = ln & 0xffff, NLEN = ln >> 16;
    if (NLEN != ((~LEN) & 0xffff)) { gs.status = E_STORED_LEN; gs.mode = GM_DONE; return; }
    u64 byte0 = st.br.pos >> 3;
    if ((byte0 + LEN) * 8 > st.limit_bit) { gs.status = SEG_OVERSHOOT; gs.mode = GM_DONE; return; }
    u64 avail = it.end_byte - byte0;
    u32 ncopy = avail < LEN ? (u32)avail : LEN;
    if (ncopy) {
      // a run of its own: one 8-word piece at the first granule at or after the block header (the block
      // is at least 35 bits long, so the piece ends before anything that follows can start)
      // (a pool of one word per two bits: a block of a few octets is too short for that — the item is declined)
      const ItemPool ip = kg_item_pool(it, P);
      const u64 x = (((gs.blk_pos >> ip.half) - ip.slot0) + 7) & ~7ull;
      const bool room = x + 8 <= ((((byte0 + ncopy) * 8) >> ip.half) & ~7ull) - ip.slot0;
      if (!room || gs.nruns + 1 > kg_run_slots(it, byte0 * 8)) { gs.status = SEG_REDO; gs.mode = GM_DONE; return; }
      u16* t = tok0 + x;
      t[0] = (u16)(TOK_STORED | (ncopy & 0x3fff));
      t[1] = (u16)((ncopy >> 14) | ((u32)(byte0 & 0x1fff) << 2));
      t[2] = (u16)((byte0 >> 13) & 0x7fff);
      t[3] = (u16)((byte0 >> 28) & 0x7fff);
      t[4] = t[5] = t[6] = t[7] = (u16)TOK_NOP;
      RunRec rr;
      rr.off8 = (u32)(x >> 3);
      rr.n8 = 1;
      rr.out = ncopy;
      rr.mdef = 0;
      if (gs.nruns == 0) gs.run0 = rr; else ip.runs[gs.nruns] = rr;
      gs.nruns += 1;
      gs.T += 8;
      gs.produced += ncopy;
    }
    if (ncopy < LEN) { gs.fail_pos = (byte0 + ncopy) * 8; gs.status = SEG_UNDERRUN; gs.cut = 2; gs.mode = GM_DONE; return; }
    gs.P = (byte0 + LEN) * 8;
    kg_block_end(gs, st, it, P, fmt, fixup);
    return;
  }
  if (btype == 3) { gs.status = E_BTYPE; gs.mode = GM_DONE; return; }
  if (btype == 1) {
    gs.P = st.br.pos;
    if (gs.tables == 1) {
      gs.mode = GM_BLOCK;
    } else {
      gs.tables = 1;
      gs.fixed = 1;
      gs.hlit = 288;
      gs.hdist = 32;
      gs.mode = GM_BUILD;
    }
    return;
  }
  if (P.hdr) {  // K1h parsed this header already
    const HdrRec h = P.hdr[idx];
    if (h.sizes && h.hdr_bit == gs.blk_pos) {
      gs.tables = 2;
      gs.hlit = h.sizes & 0xffffu;
      gs.hdist = h.sizes >> 16;
      gs.fixed = 2;
      gs.P = h.end_bit;
      gs.mode = GM_BUILD;
      return;
    }
  }
  const i32 e = kg_dynamic_header(gt, gs, st);
  gs.tables = 2;
  if (e) {
    gs.status = e;
    gs.fail_pos = st.fail_pos;
    gs.mode = GM_DONE;
    return;
  }
  gs.fixed = 0;
  gs.P = st.br.pos;
  gs.mode = GM_BUILD;
}

template <int G>
TBZ_DEV void k1g_body(const K1gParams& P, KgLds<G>& S) {
  constexpr u32 NG = 64 / G;
  const u32 lane = tbz_lane();
  const u32 gang = lane / G, g = lane % G, base = lane - g;
  const bool leader = g == 0;
  const u32 idx = tbz_block() * NG + gang;
  const bool have = idx < P.n_items;
  typename KgLds<G>::GT& gt = S.gt[gang];
  GangState& gs = S.gs[gang];
  Item it{};
  if (have) it = P.items[idx];
  const u32 fmt = (it.flags >> ITEM_FMT_SHIFT) & 3;
  const bool fixup = (it.flags & ITEM_FIXUP) != 0;
  // (a launch of gangs of 64 BESIDE a narrow one — P.only_wide — takes the items longer than wide_bits and nothing else:
  // one item per wave, so the whole workgroup leaves)
  if (G == 64 && P.only_wide) {
    const u64 lim = (it.end_byte * 8 < it.limit_bit) ? it.end_byte * 8 : it.limit_bit;
    if (!have || (it.flags & ITEM_FIXUP) || !(lim > it.start_bit && lim - it.start_bit > P.wide_bits)) return;
  }
  const ItemPool ip = kg_item_pool(it, P);
  const u32 half = ip.half;
  const u64 slot0 = ip.slot0;
  u16* tok0 = ip.tok;
  K1State st;
  br_init(st.br, P.in_base, it.end_byte, S.inbuf, KgShape<G>::INBUF);
  // the gang's canonical lists: built in `bc` (LDS: the gang's share of the input windows, dead while a code is built —
  // or a place of their own for narrow gangs), read by the exact step from `gc` (the item's scratch in memory, or `bc`)
  constexpr bool COLD_IN_LDS = KgLds<G>::COLD_IN_LDS;
  GangCold* bc;
  const GangCold* gc;
  if constexpr (COLD_IN_LDS) {
    bc = &S.c.cold[gang];
    gc = bc;
  } else {
    static_assert(sizeof(S.inbuf) / NG >= sizeof(GangCold), "a gang's share of the windows holds its canonical lists");
    bc = (GangCold*)((u8*)S.inbuf + gang * (sizeof(S.inbuf) / NG));
    gc = (const GangCold*)(P.cold + (u64)(have ? idx : 0) * KG_COLD_STRIDE);
  }
  st.end_bit = it.end_byte * 8;
  st.limit_bit = fixup ? ~0ull : it.limit_bit;
  st.produced = 0;
  st.deficit = 0;
  st.hist0 = 0;
  st.viol_out = ~0ull;
  st.tok0 = tok0;
  st.tok = tok0;
  st.fail_pos = it.start_bit;
  const u64 lim64 = st.end_bit < st.limit_bit ? st.end_bit : st.limit_bit;
  [[maybe_unused]] const u64 tr_t0 = TBZ_TR_NOW();
  [[maybe_unused]] u64 tr_hdr = 0, tr_build = 0, tr_round = 0, tr_commit = 0, tr_n = 0, tr_a = 0, tr_b = 0, tr_first = 0, tr_wt1 = 0, tr_li1 = 0, tr_ph1 = 0, tr_wt2 = 0, tr_li2 = 0;

  // a gzip header with a header CRC (FHCRC): the gang builds the CRC table in its (still unused) lookup-table LDS first,
  // and if there is an extra field (up to 65 535 octets: one lane took 10 ms over a false `1f 8b 08` candidate's) its
  // lanes take the field's CRC in parallel: lane g its piece, the leader the ordered combine
  const u32* crc_tab = nullptr;
  GzExtraCrc xc{0, 0, 0};
  {
    bool hc = false;
    if (have && (it.flags & ITEM_HEAD) && fmt == 2 && (it.start_bit >> 3) + 4 <= it.end_byte) hc = (P.in_base[(it.start_bit >> 3) + 3] & 2) != 0;
    if (hc) {
      u32* tab = (u32*)gt.lfast;
      for (u32 n = g; n < 256; n += G) {
        u32 c = n;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (0xedb88320u ^ (c >> 1)) : (c >> 1);
        tab[n] = c;
      }
      crc_tab = tab;
    }
    tbz_sync();
    const u64 b0 = it.start_bit >> 3;
    u32 xlen = 0;
    if (hc && b0 + 12 <= it.end_byte && (P.in_base[b0 + 3] & 4)) xlen = (u32)P.in_base[b0 + 10] | ((u32)P.in_base[b0 + 11] << 8);
    const bool par = hc && xlen >= 256 && b0 + 12 + xlen <= it.end_byte;  // (gang-uniform)
    u32 piece = 0, plen = 0, xp = 0;
    if (par) {
      const u32 chunk = (xlen + G - 1) / G;
      const u32 lo_ = g * chunk < xlen ? g * chunk : xlen, hi_ = lo_ + chunk < xlen ? lo_ + chunk : xlen;
      const u8* q = P.in_base + b0 + 12;
      for (u32 i = lo_; i < hi_; i++) piece = (piece >> 8) ^ crc_tab[(piece ^ q[i]) & 0xffu];
      plen = hi_ - lo_;
      // x^(8 * plen) by squaring (x^1 = 0x40000000 in this reflected form, so x^8 = 0x00800000)
      u32 pw = 0x80000000u, sq = 0x00800000u;
      for (u32 n = plen; n; n >>= 1) {
        if (n & 1) pw = crc_mulmod(sq, pw);
        sq = crc_mulmod(sq, sq);
      }
      xp = pw;
    }
    // ordered combine over the gang's lanes (a loop of shuffles: every lane of the wave takes part)
    u32 acc = 0, accp = 0x80000000u;
    if (tbz_ballot(par) != 0) {
      for (u32 k = 0; k < (u32)G; k++) {
        const u32 pk_ = tbz_shfl(piece, (int)(base + k)), xk = tbz_shfl(xp, (int)(base + k)), nk = tbz_shfl(plen, (int)(base + k));
        if (par && nk) {
          acc = crc_mulmod(xk, acc) ^ pk_;
          accp = crc_mulmod(xk, accp);
        }
      }
      if (par) {
        xc.valid = 1;
        xc.raw = acc;
        xc.xpow = accp;
      }
    }
  }
  if (leader) {
    gs.P = it.start_bit;
    gs.T = 0;
    gs.produced = 0;
    gs.blk_pos = it.start_bit;
    gs.blk_prod = 0;
    gs.blk_tok = 0;
    gs.fail_pos = it.start_bit;
    gs.status = 0;
    gs.cut = 0;
    gs.mode = have ? GM_HEADER : GM_DONE;
    gs.bfinal = 0;
    gs.deficit = 0;
    gs.tables = 0;
    gs.land = 0xFFFFFFFFu;
    gs.tr0 = gs.tr1 = gs.tr_have = 0;
    gs.hlit = gs.hdist = gs.fixed = 0;
    gs.nruns = gs.blk_runs = 0;
    gs.run0 = RunRec{};
    gs.rounds = gs.valid_lanes = 0;
    gs.inl = gs.noinline = 0;
    gs.ptry = 0;
    gs.min_len = 0;
    // (an item far larger than any block an encoder emits holds several: a first guess, replaced after the first block)
    gs.est = (have && !fixup && lim64 > it.start_bit && lim64 - it.start_bit >= KG_MULTI_BLOCK_BITS) ? KG_BLOCK_GUESS_BITS : 0u;
    if (G < 64 && have && !fixup && P.wide_bits && lim64 > it.start_bit && lim64 - it.start_bit > P.wide_bits) {
      gs.status = SEG_WIDE;  // the gang width follows the launch's MEAN item: this one would be the kernel's straggler
      gs.mode = GM_DONE;
    } else
    if (have && (it.flags & ITEM_HEAD)) {
      br_seek_fill(st.br, it.start_bit);
      i32 e = k1_container_header(st, fmt, crc_tab, false, &xc);
      if (e) {
        gs.status = e;
        gs.fail_pos = st.fail_pos;
        gs.mode = GM_DONE;
      }
      gs.P = st.br.pos;
      if (!e && !fixup && gs.P == st.limit_bit) {  // the first block is itself a candidate (K0b): header only
        gs.status = SEG_LANDED;
        gs.mode = GM_DONE;
      }
    }
  }

  for (;;) {
    tbz_sync();
    if (tbz_ballot(gs.mode != GM_DONE) == 0) break;
    // ---- H: leaders whose gang is between blocks parse the next header
    tr_a = TBZ_TR_NOW();
    if (leader && gs.mode == GM_HEADER) {
      kg_leader_header(gt, gs, st, it, P, tok0, fmt, fixup, idx);
      // a continuation inside a block: the header has been read, the tokens go on where the session stopped
      if ((it.flags & ITEM_RESUME) && gs.blk_pos == it.start_bit && (gs.mode == GM_BUILD || gs.mode == GM_BLOCK) && P.resume_bit > gs.P)
        gs.P = P.resume_bit;
    }
    tbz_sync();
    tr_b = TBZ_TR_NOW();
    tr_hdr += tr_b - tr_a;
    // ---- B: gangs with a new code build it together (wave-uniform branch: collectives inside)
    const bool building = gs.mode == GM_BUILD;
    if (tbz_ballot(building) != 0) {
      const u32 nl = building ? gs.hlit : 0, nd = building ? gs.hdist : 0;
      if (building && gs.fixed == 2) {  // the code lengths K1h decoded
        const u8* src = P.hdr_lens + (u64)idx * K1_SCRATCH;
#pragma nounroll
        for (u32 i = g * 4; i < 320; i += G * 4) *(u32*)(kg_lens(gt) + i) = *(const u32*)(src + i);
      } else if (building && gs.fixed)  // fixed code lengths: huffman-tree.lisp:89-97
#pragma nounroll
        for (u32 i = g; i < 320; i += G) kg_lens(gt)[i] = (u8)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
      tbz_sync();
      st.br.bw = 1ull << 62;  // (the windows are the builders' scratch: whoever reads next reloads)
      const i32 e1 = kg_build<G, KG_TBL, KgPools<G>::L, true, u16>(kg_lens(gt), nl, bc->lsym, bc->llim, bc->ldlt, gt.lfast, g, base);
      const i32 e2 = kg_build<G, KG_TBD, KgPools<G>::D, false, u8>(kg_lens(gt) + nl, nd, bc->dsym, bc->dlim, bc->ddlt, gt.dfast, g, base);
      tbz_sync();
      if constexpr (!COLD_IN_LDS) {  // park the lists in the item's scratch (the gang's lanes, a dword each)
        if (building) {
          const u32* src = (const u32*)bc;
          u32* dst = (u32*)(P.cold + (u64)idx * KG_COLD_STRIDE);
#pragma nounroll
          for (u32 i = g; i < sizeof(GangCold) / 4; i += G) dst[i] = src[i];
          if (leader) gs.min_len = bc->llim[15] | (bc->dlim[15] << 8);
        }
        tbz_sync();
      } else if (leader && building) {
        gs.min_len = bc->llim[15] | (bc->dlim[15] << 8);
      }
      if (leader && building) {
        const i32 e = e1 ? e1 : e2;
        if (e) {
          gs.status = e;
          gs.mode = GM_DONE;
        } else {
          gs.mode = GM_BLOCK;
        }
      }
      tbz_sync();
    }
    // ---- R: one round for the gangs that are inside a Huffman block
    tr_a = TBZ_TR_NOW();
    tr_build += tr_a - tr_b;
    const bool inblk = gs.mode == GM_BLOCK;
    const u64 Pb = gs.P;
    RoundOut ro;
    ro.c = ~0ull;
    ro.e = 0;
    ro.aux = 0;
    ro.n = 0;
    ro.out = 0;
    ro.mdef = -(1 << 30);
    ro.flag = RF_JUNK;
    ro.hdr = 0;
    ro.nhdr = 0;
    ro.assumed = 0;
    ro.bf_end = -1;
#ifdef TBZ_WAVE_TRACE
    ro.li = 0;
    if (lane == 0) S.tr_cnt[0] = S.tr_cnt[1] = 0;
    tbz_sync();
#endif
    // consecutive fixed-Huffman blocks are decoded through (not by repair items: they land on a marker after EVERY block)
    const bool inl_on = inblk && gs.tables == 1 && !fixup && !gs.noinline;
    u16* stage = P.tok;
    u64 s_lo = 0;  // this lane's region: words from the item's token base
    // sub-range per lane: what is left of the item split evenly (the next marker is where it should end)
    u32 sub = P.sub_min;
    if (inblk) {
      u64 remb = lim64 > Pb ? lim64 - Pb : 0;
      if (gs.est) {  // what is left of the block if it is as long as the one before it (+ 1/8), else a quarter more
        const u64 used = Pb - gs.blk_pos;
        const u64 left = gs.est > used ? (u64)gs.est - used + (gs.est >> 3) : (u64)(gs.est >> 2);
        remb = remb < left ? remb : left;
      }
      const u64 per = (remb + G - 1) / G;
      sub = per >= KG_SUB_MAX ? KG_SUB_MAX : (u32)per;
      sub = (sub + 63) & ~63u;
      sub = sub < P.sub_min ? P.sub_min : sub;
    }
    const u64 s_g = Pb + (u64)g * sub;
    // a periodic stretch (see kg_periodic): the lanes before the first one whose piece of the bitstream is not T-periodic
    // start exactly on a token, with no run-up
    u64 pstart = 0;
    const bool ptry = inblk && gs.ptry != 0;
    if (tbz_ballot(ptry) != 0) {  // wave-uniform: collectives inside
      u32 T = 0;
      if (ptry) T = kg_token_bits(gt, st.br, Pb, lim64);
      const bool okp = ptry && T != 0 && (g == 0 || kg_periodic(st.br, s_g - sub, s_g + 64, T, lim64));
      const u64 okm = (tbz_ballot(okp) >> base) & (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1));
      const u32 f = okm == (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) ? (u32)G : (u32)__builtin_ctzll(~okm);
      if (ptry && g != 0 && g < f) pstart = Pb + ((s_g - Pb + T - 1) / T) * T;
    }
    if (inblk) {
      const u64 start = g == 0 ? Pb : pstart ? pstart : (s_g - Pb > P.ovl ? s_g - P.ovl : Pb);
      s_lo = ((s_g >> half) & ~7ull) - slot0;
      stage = tok0 + s_lo;  // private region of the token pool: [slot(s_g), slot(s_g + sub)), 16-octet aligned
      Inl il;
      il.on = inl_on;
      il.cur_bf = g == 0 ? (i32)gs.bfinal : -1;
      kg_lane_round(gt, *gc, st.br, start, pstart ? pstart : s_g, s_g + sub, lim64, stage, S.tokring + lane * KG_RING_STRIDE, (sub >> half) - 16, ro, il);
    }
    tr_b = TBZ_TR_NOW();
    tr_round += tr_b - tr_a;
    if (tr_n == 0) tr_first = tr_b - tr_a;
#ifdef TBZ_WAVE_TRACE
    {
      tbz_sync();
      u32 mx = S.tr_cnt[0], sm = ro.li, pm = S.tr_cnt[1];
      for (int m = 1; m < 64; m <<= 1) sm += tbz_shfl_xor(sm, m);
      if (tr_n == 0) { tr_wt1 = mx; tr_li1 = sm; tr_ph1 = pm; } else { tr_wt2 += mx; tr_li2 += sm; }
    }
#endif
    tr_n++;
    // ---- chain validation: lane g counts iff it began recording exactly where lane g-1 stopped
    const u32 pe_lo = tbz_wave_shr1((u32)ro.e), pe_hi = tbz_wave_shr1((u32)(ro.e >> 32));
    const u64 prev_e = ((u64)pe_hi << 32) | pe_lo;
    const u32 prev_flag = tbz_wave_shr1(ro.flag);
    const bool link = inblk && ro.flag != RF_JUNK && (g == 0 || (ro.c == prev_e && prev_flag == RF_STOP));
    const u64 okm = tbz_ballot(link);
    constexpr u64 GMASK = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1);
    const u64 gm = (okm >> base) & GMASK;
    u32 v = gm == GMASK ? (u32)G : (u32)__builtin_ctzll(~gm);  // valid lanes of my gang
    // lanes that decoded through block headers: BFINAL of the block each lane STARTED in is the last one reported
    // before it along the chain (the leader's for lane 0); a lane that took an unknown block for non-final and went
    // through its end-of-block code was wrong if that block was the final one: the round ends before that lane
    i32 bf_last = -1;       // BFINAL reported by the last lane of the committed chain that passed a header
    u64 hdr_last = 0;
    bool any_hdr = false;
    if (tbz_ballot(ro.nhdr != 0) != 0) {  // wave-uniform
      i32 bf_in = ro.bf_end;  // inclusive scan "last defined" over the gang's lanes, then shifted by one
#pragma unroll
      for (u32 d = 1; d < (u32)G; d <<= 1) {
        const i32 t = (i32)tbz_shfl_up((u32)bf_in, d);
        if (g >= d && bf_in < 0) bf_in = t;
      }
      const i32 incl = bf_in;
      i32 before = (i32)tbz_wave_shr1((u32)incl);
      if (g == 0) before = -1;
      const i32 start_bf = before < 0 ? (i32)gs.bfinal : before;
      const u64 bad = (tbz_ballot(inblk && ro.assumed && start_bf == 1) >> base) & GMASK;
      if (bad) {
        const u32 fb = (u32)__builtin_ctzll(bad);
        v = v < fb ? v : fb;
      }
      const u32 lvv = base + (v ? v - 1 : 0);
      const i32 bf_lv = (i32)tbz_shfl((u32)incl, (int)lvv);
      bf_last = v ? bf_lv : -1;
      // the last header passed by a committed lane
      u64 hp = (g < v && ro.nhdr) ? ro.hdr : 0;
#pragma unroll
      for (int m = 1; m < G; m <<= 1) {
        const u64 t = tbz_shfl_xor64(hp, m);
        hp = t > hp ? t : hp;
      }
      hdr_last = hp;
      any_hdr = hp != 0;
      if (leader && inblk) gs.noinline = bad ? 1u : 0u;
    } else if (leader && inblk) {
      gs.noinline = 0;
    }
    const bool valid = g < v;
    // ---- commit: nothing is copied.  A valid lane's tokens stay where it staged them; it pads them to
    // the 8-word granule and enters them in the item's run table, which is what K2 follows.
    const u32 n8 = (ro.n + 7) >> 3;
    const bool hasrun = valid && ro.n != 0;
    const u32 nn = hasrun ? n8 * 8 : 0, oo = valid ? ro.out : 0, hr = hasrun ? 1u : 0u;
    const u32 in_n = tbz_wave_incl_scan_u32(nn), in_o = tbz_wave_incl_scan_u32(oo), in_r = tbz_wave_incl_scan_u32(hr);
    const int below = base ? (int)base - 1 : 0;
    const u32 bn = tbz_shfl(in_n, below), bo = tbz_shfl(in_o, below), br_ = tbz_shfl(in_r, below);
    const u32 base_n = base ? bn : 0, base_o = base ? bo : 0, base_r = base ? br_ : 0;
    const u32 PO = in_o - oo - base_o, rank = in_r - hr - base_r;
    const u32 tot_n = tbz_shfl(in_n, (int)(base + G - 1)) - base_n;
    const u32 tot_o = tbz_shfl(in_o, (int)(base + G - 1)) - base_o;
    const u32 tot_r = tbz_shfl(in_r, (int)(base + G - 1)) - base_r;
    const u32 lv = base + (v ? v - 1 : 0);
    const u64 e_last = tbz_shfl64(ro.e, (int)lv), aux_last = tbz_shfl64(ro.aux, (int)lv);
    const u32 flag_last = tbz_shfl(ro.flag, (int)lv);
    // the last run must end before the granule in which the next thing (a round, a stored run) may start,
    // and the table must not outgrow the item's span; else the item is left to the one-lane kernel
    const u64 end_lv = tbz_shfl64(s_lo + nn, (int)lv);
    const bool fits = !inblk || (end_lv <= ((e_last >> half) & ~7ull) - slot0 && gs.nruns + tot_r <= kg_run_slots(it, e_last));
    if (hasrun && fits) {  // (the lane has padded its run to the granule already)
      RunRec rr;
      rr.off8 = (u32)(s_lo >> 3);
      rr.n8 = n8;
      rr.out = ro.out;
      rr.mdef = ro.mdef > 0 ? (u32)ro.mdef : 0u;
      const u32 k = gs.nruns + rank;
      if (k == 0) gs.run0 = rr; else ip.runs[k] = rr;
    }
    // history check material: largest (distance - octets produced before the match) over the round
    u64 hb = gs.produced + PO;
    i32 hbase = hb > (1u << 30) ? (1 << 30) : (i32)hb;
    i32 cand = (valid && ro.mdef > -(1 << 29)) ? ro.mdef - hbase : -(1 << 30);
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
      i32 t = (i32)tbz_shfl_xor((u32)cand, m);
      cand = t > cand ? t : cand;
    }
    tbz_sync();
    if (leader && inblk && !fits) {
      gs.status = SEG_REDO;
      gs.mode = GM_DONE;
    } else if (leader && inblk) {
      gs.rounds += 1;
      gs.valid_lanes += v;
      gs.ptry = (v <= 2 && flag_last == RF_STOP) ? 1u : 0u;  // (inside a block, and next to nothing committed)
      if (any_hdr) {  // the chain went through block headers: the current block is the last of them
        if (bf_last >= 0) gs.bfinal = (u32)bf_last;
        gs.blk_pos = hdr_last;
        gs.inl = 1;
      }
      gs.T += tot_n;
      gs.nruns += tot_r;
      gs.produced += tot_o;
      if (cand > 0 && (u32)cand > gs.deficit) gs.deficit = (u32)cand;
      if (flag_last == RF_STOP) {
        gs.P = e_last;
      } else if (flag_last == RF_EOB) {
        gs.P = e_last;
        if (!gs.inl) {
          const u64 bb = e_last - gs.blk_pos;
          gs.est = bb > 0x7fffffffull ? 0x7fffffffu : (u32)bb;
        }
        kg_block_end(gs, st, it, P, fmt, fixup);
      } else if (flag_last == RF_LIMIT) {
        gs.fail_pos = e_last;
        gs.status = aux_last > st.end_bit ? SEG_UNDERRUN : SEG_OVERSHOOT;
        gs.mode = GM_DONE;
      } else if (flag_last == RF_SYM) {
        gs.status = E_INVALID_CODE;
        gs.mode = GM_DONE;
      } else {  // unassigned bit pattern: error unless the input ends inside the bits the reference needs
        u32 need = flag_last == RF_CODE_LIT ? (gs.min_len & 0xffu) : (gs.min_len >> 8);
        if (aux_last + need > st.end_bit) {
          gs.fail_pos = e_last;
          gs.status = SEG_UNDERRUN;
        } else {
          gs.status = E_INVALID_CODE;
        }
        gs.mode = GM_DONE;
      }
    }
    tr_commit += TBZ_TR_NOW() - tr_b;
  }
#ifdef TBZ_WAVE_TRACE
  if (P.trace && lane == 0) {
    u64* t = P.trace + (u64)tbz_block() * 16;
    u32 xcc = 0, hwid = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    t[0] = tr_t0;
    t[1] = TBZ_TR_NOW();
    t[2] = ((u64)xcc << 32) | hwid;
    t[3] = tr_hdr + tr_commit;
    t[4] = tr_build;
    t[5] = tr_round;
    t[6] = tr_first;
    t[7] = tr_n;
    t[8] = tr_wt1; t[9] = tr_li1; t[10] = tr_ph1; t[11] = tr_wt2; t[12] = tr_li2;
  }
#endif

  if (leader && have) {
    SegResult r;
    if (gs.status == SEG_OVERSHOOT && gs.inl) gs.status = SEG_REDO;  // the block's start lies inside a run: one lane redoes the item
    if (gs.status == SEG_OVERSHOOT) {
      r.end_bit = gs.blk_pos;
      r.out_bytes = gs.blk_prod;
      r.tok_words = gs.blk_tok;
      r.n_runs = gs.blk_runs;
    } else {
      r.end_bit = gs.status == SEG_UNDERRUN ? gs.fail_pos : gs.P;
      r.out_bytes = gs.produced;
      r.tok_words = gs.T;
      r.n_runs = gs.nruns;
    }
    r.pad = (gs.status == SEG_UNDERRUN && gs.fail_pos == gs.blk_pos) ? 1u : gs.status == SEG_UNDERRUN ? gs.cut : 0u;
    r.tok = (u64)tok0;
    r.runs = (u64)ip.runs;
    r.run0 = gs.run0;
    r.status = gs.status;
    r.max_deficit = gs.deficit;
    r.trailer0 = gs.tr0;
    r.trailer1 = gs.tr1;
    r.trailer_have = gs.tr_have;
    r.land_marker = gs.land;
    r.reserved = ((u64)gs.rounds << 32) | gs.valid_lanes;
    if (gs.status == SEG_UNDERRUN) {
      // where a resumed decode would start: the block in which the input ran out, and what came out before it
      // (after blocks decoded THROUGH, only the item's own start is known exactly: land_marker = 1)
      r.trailer0 = (u32)gs.blk_pos;
      r.trailer1 = (u32)(gs.blk_pos >> 32);
      r.reserved = gs.blk_prod;
      r.land_marker = gs.inl ? 1u : 0u;
    }
    P.res[idx] = r;
  }
}

#define TBZ_K1G_KERNEL(G, OCC)                                     \
  TBZ_KERNEL_OCC(OCC) void tbz_k1g##G##_huff_decode(K1gParams P) { \
    TBZ_SHARED KgLds<G> S;                                  \
    k1g_body<G>(P, S);                                      \
  }
TBZ_K1G_KERNEL(8, 3)
TBZ_K1G_KERNEL(16, 3)
// (round 4: the gangs of 32 too — 9.9 KB since their canonical lists left the LDS and the windows are twelve words)
TBZ_K1G_KERNEL(32, 4)
// (gangs of 64 have one gang's tables per workgroup — 9.8 KB of LDS, sixteen workgroups per CU — so four waves per SIMD
// is theirs to have if the registers allow: 128 instead of 146; config 3's 4 096 members are then ONE generation of
// workgroups, K1 3.45 -> 2.82 ms.  The narrower gangs are held at three per SIMD by their LDS.)
TBZ_K1G_KERNEL(64, 4)
#undef TBZ_K1G_KERNEL

// ================================================================================================
// K2 — LZ77 resolve: tokens -> LDS window -> coalesced 16-byte stores.  One workgroup per group.
//
// A batch is up to 128 token words, two per lane.  Lanes classify their words (literal / match head / payload) with
// ballots, a DPP prefix sum gives every token its output offset, literals are stored at once, and
// matches are resolved LANE-PARALLEL in rounds: a match is ready when the part of its source that
// it does not produce itself lies below the high-water mark (the offset of the first unresolved
// match; everything below is final).  The first unresolved match is always ready, so every round
// makes progress; typical text needs 2-4 rounds per batch.  Long matches (> 32 octets) and stored
// runs are copied cooperatively by all 64 lanes.  Replaces copy-history / out-byte / :copy-block
// (deflate.lisp:233-359, :538-573).
//
// Two windows:
//   LINEAR  a group whose whole output fits the LDS (up to 32 KiB: flush-delimited segments) keeps every octet at
//           window[a0 + offset]: no wrap arithmetic, one flush at the end;
//   RING    any other group runs through a SMALL ring: K2R_HIST octets of history plus the batches in flight (11 KB
//           instead of the 36 KB a whole deflate window takes: ten workgroups per CU instead of four).  The ring is
//           flushed every K2R_FLUSH octets, and a match whose distance exceeds K2R_HIST copies from the OUTPUT the
//           group has already flushed (L2-resident: written a few microseconds earlier by the same workgroup) —
//           always final, so such matches are resolved first, in one round of wide loads.
// Groups that need history they do not hold (H-groups, see K6) run through the ring kernel twice — K2's copies are the
// same whatever the octets are — once per PLANE (octets -> out, marks -> the mark plane), as neighbouring workgroups
// that read the same tokens; a source before the group's first octet is a pointer computed on the spot (nothing to
// initialise), and a far source comes from the plane's own flushed output.  (Both planes in one workgroup — two rings
// moved by the same copies — was built and measured: 26.6 KB of LDS, six workgroups per CU, 8.4 ms per GiB against
// 6.4 ms for two passes at ten per CU: profiles/README.md.)
//
// The resolve step, in the order of the file: k2_copy_coop (one match, all lanes); k2_short_store / k2_short_copy /
// k2_short_octets (one match, its own lane); k2_far_round (round 0 of the ring kernels); k2_rounds (the one round loop,
// both windows); k2_resolve, the driver over the two.
// ================================================================================================
constexpr u32 ADLER_P = 65521;
#ifndef TBZ_EXP_K2R_SPAN  // (experiments: hipcc -DTBZ_EXP_K2R_SPAN=768 -DTBZ_EXP_K2R_HIST=4096 -DTBZ_EXP_K2R_FLUSH=1024 ...)
#define TBZ_EXP_K2R_SPAN 1536
#endif
#ifndef TBZ_EXP_K2R_HIST
#define TBZ_EXP_K2R_HIST 8192
#endif
#ifndef TBZ_EXP_K2R_FLUSH
#define TBZ_EXP_K2R_FLUSH 2048
#endif
constexpr u32 K2L_SPAN = 3072;   // linear windows: most octets of a stored run copied between two flush checks
constexpr u32 K2R_SPAN = TBZ_EXP_K2R_SPAN;   // ring kernels on two / three waves: most octets one batch may produce (batches are in flight)
constexpr u32 K2_SPAN = 2 * K2R_SPAN;        // (one-wave ring kernel) most octets one batch may produce
constexpr u32 K2R_HIST = TBZ_EXP_K2R_HIST;   // ring kernels: a match up to this distance copies inside the ring, a longer one from the output
constexpr u32 K2R_FLUSH = TBZ_EXP_K2R_FLUSH; // ring kernels: flush every this many octets (what a far match reads must have left the ring:
                                 // K2R_HIST >= K2R_FLUSH + K2_SPAN + 258 + 16)
constexpr u32 K2_SHORT = 32;     // matches up to this length are copied by their own lane
constexpr u32 K2_TCH = 512;      // token words per staged chunk: one 16-octet load per lane
constexpr u32 K2_TOKBUF = 2 * K2_TCH;  // LDS token ring: the chunk in use + the next one (prefetched a chunk ahead)
constexpr u32 K2_SLACK = 64;     // window octets past a group's output: alignment (16) + room for wide reads
constexpr u32 K2_SMALL_MAX = 32768;  // groups producing at most this much (incl. K2_SLACK) take the linear path
constexpr u32 K2_IDT = 256 + 40; // identity octets (k & 255): the low plane of a run of computed pointers, read like any source
static_assert(K2R_HIST >= K2R_FLUSH + K2_SPAN + 258 + 16 + K2R_SPAN, "far sources must have been flushed");
static_assert(K2R_FLUSH > K2R_SPAN, "a flush interval above the batch span: the first batch alone never triggers a flush");

// window flavours: RW = 0 is the linear window; otherwise a ring of RW octets (a multiple of 16) of which HIST are
// history
template <u32 RW_, u32 HIST_>
struct K2W {
  static constexpr u32 RW = RW_, HIST = HIST_;
  static constexpr bool LINEAR = RW_ == 0;
};
using K2Linear = K2W<0, 0>;
constexpr u32 K2R_RW = K2R_HIST + K2_SPAN + 64;  // history + two spans (one-wave kernel: one span of twice the size)
static_assert(K2R_RW % 16 == 0 && K2_SPAN == 2 * K2R_SPAN, "16-octet chunks must not straddle the ring's seam");
using K2Ring = K2W<K2R_RW, K2R_HIST>;

struct K2Params {
  const Seg* segs;    // (a segment names its tokens and run table by address: the call's pools, the repair launches', an item's own)
  const Group* groups;
  const u32* order;   // group indices this launch handles
  const u8* in_base;  // source of stored runs
  u8* out_base;
  u32 n_groups;       // entries in `order` (order == nullptr: groups 0..n_groups-1, filtered by `cls`)
  u32 win_bytes;      // LINEAR launches: octets of the window (dynamic LDS = win_bytes + 2*K2_TOKBUF)
  u32 cls;            // with order == nullptr: 1 = only groups that fit the linear window, 2 = only the others
  CkPartial* gck;     // two-wave kernel: adler32 partial of every group's output, computed from the window while it
  CkChunk* gchunks;   //   is flushed (nullptr: not wanted); gchunks[g].len = octets the group stored
  // ---- groups decoded against a SYMBOLIC history (ring kernels only; SURVEY §8f-1, see K6 below)
  u32 hist;           // 1: the 32 KiB before the group's first octet are not known: a source there is a POINTER
  u32 plane;          // 0: octets (a pointer's low octet where the source is symbolic) -> out_base
                      // 1: 0 for a known octet, 0x80 | pointer >> 8 for a symbolic one    -> out_base = the mark plane
  u64 out_bias;       // octet x of the output lives at out_base[x - out_bias] (the mark plane covers the streams' extent only)
  // ---- ring launches that take plain groups and both planes of the H-groups together (k2_ring_select): workgroups
  // [0, n_plain) handle order[0 .. n_plain), workgroup n_plain + 2k + q handles plane q of order[n_plain + k]
  u32 mixed;          // 1: that mapping (hist / plane / out_base / out_bias above are then per workgroup, taken from below)
  u32 n_plain;
  u8* mark_base;
  u64 mark_bias;
  // ---- launches over a RANGE of the device-built tables (order == nullptr): workgroup b handles group first + b, and
  // n_groups is the END of the range; segs / groups / gck / gchunks stay indexed by the group's own number
  u32 first;
};

template <class W>
TBZ_DEV u32 ring(u32 x) { return W::LINEAR ? x : (x >= W::RW ? x - W::RW : x); }  // x < 2 * RW

// store window[from..to) (group-relative octet offsets) to out, clipped at `clip`; `a0` = (address of
// the group's first octet) & 15 so that window index == address (mod 16) and 16-byte chunks are aligned
template <class W>
TBZ_DEV void k2_flush(const u8* win, u8* outp, u64 from, u64 to, u64 clip, u32 a0) {
  constexpr bool LINEAR = W::LINEAR;
  constexpr u32 RW = LINEAR ? 1u : W::RW;
  if (to > clip) to = clip;
  if (from >= to) return;
  const u32 lane = tbz_lane();
  tbz_sync();
  u64 head_end = ((from + a0 + 15) & ~15ull) - a0;  // first 16-aligned offset >= from
  if (head_end > to) head_end = to;
  u64 body_end = head_end + ((to - head_end) & ~15ull);
  // window index of offset x >= from: one 64-bit remainder per call, the rest in 32 bits (to - from < 2^32 always)
  const u32 rf = LINEAR ? (u32)(from + a0) : (u32)((from + a0) % RW);
  auto idx = [&](u64 x) -> u32 { return LINEAR ? rf + (u32)(x - from) : (rf + (u32)(x - from)) % RW; };
  if (from + lane < head_end) outp[from + lane] = win[idx(from + lane)];
  u64 nchunk = (body_end - head_end) >> 4;
  const u32 r0 = idx(head_end);
  for (u32 c = lane; c < (u32)nchunk; c += 64) {
    u32 ri = LINEAR ? r0 + c * 16 : (r0 + c * 16) % RW;
    uint4 v = *(const uint4*)(win + ri);
    *(uint4*)(outp + head_end + (u64)c * 16) = v;
  }
  if (body_end + lane < to) outp[body_end + lane] = win[idx(body_end + lane)];
  tbz_sync();
}

// what a resolve step needs to know about the group beyond the window
struct K2Src {
  u8* win;
  const u8* idt;    // RING: K2_IDT identity octets (the octet plane of computed pointers)
  const u8* g0;     // RING: the group's first octet in the output plane this workgroup writes (far sources)
  u32 hist, plane;  // RING: K2Params::hist / plane of this workgroup
};

// window index of the group-relative offset t, given that offset `gpos` sits at index `rpos` (|t - gpos| < RW)
template <class W>
TBZ_DEV u32 k2_index(u32 rpos, u64 gpos, i64 t) {
  if (W::LINEAR) return (u32)((i64)rpos + (t - (i64)gpos));
  const i64 dlt = t - (i64)gpos;
  return dlt >= 0 ? ring<W>(rpos + (u32)dlt) : (rpos >= (u32)(-dlt) ? rpos - (u32)(-dlt) : rpos + W::RW - (u32)(-dlt));
}
// eight mark octets of the pointers q, q+1, ... (0x80 | index >> 8; the high part steps where the low octet wraps)
TBZ_DEV u64 k2_mark8(u32 q) {
  const u32 hi = 0x80u | (q >> 8), nb = 256 - (q & 255);
  const u64 v = (u64)hi * 0x0101010101010101ull;
  return nb < 8 ? v + (0x0101010101010101ull << (8 * nb)) : v;
}

// One match copied by all 64 lanes, whatever its source: l octets to group-relative offset d (window index rd), from
// distance dd.  An overlapping copy (dd < l) repeats the dd-octet pattern (the special cases of deflate.lisp:281-334).
// Sources: inside the window; RING: octets the group flushed earlier (distance beyond HIST); H-groups: before the group's
// first octet = a computed pointer.  Everything the copy reads is final (the caller's readiness rule).
template <class W>
TBZ_DEV void k2_copy_coop(const K2Src& S, u32 rpos, u64 gpos, i64 d, u32 rd, u32 dd, u32 l) {
  constexpr bool LINEAR = W::LINEAR;
  const u32 lane = tbz_lane();
  const i64 s = d - (i64)dd;
  u8* win = S.win;
  const bool inwin = LINEAR || (dd <= W::HIST && (!S.hist || s >= 0));
  if (inwin) {
    const u32 rs = LINEAR ? (rd >= dd ? rd - dd : 0) : (rd >= dd ? rd - dd : rd + W::RW - dd);
    if (dd >= l) {  // disjoint
      if (LINEAR || (rs + l <= W::RW && rd + l <= W::RW)) {  // 4-octet pieces, then the tail
        const u32 np = l >> 2;
        for (u32 j = lane; j < np; j += 64) {
          k2_st32(win + rd + 4 * j, k2_ld32(win + rs + 4 * j));
        }
        if (lane < (l & 3)) {
          win[rd + 4 * np + lane] = win[rs + 4 * np + lane];
        }
        return;
      }
      for (u32 j = lane; j < l; j += 64) {
        win[ring<W>(rd + j)] = win[ring<W>(rs + j)];
      }
      return;
    }
    float inv = 1.0f / (float)dd;
    for (u32 j = lane; j < l; j += 64) {
      u32 q = (u32)((float)j * inv);
      i32 r = (i32)j - (i32)(q * dd);
      if (r < 0) r += (i32)dd;
      if (r >= (i32)dd) r -= (i32)dd;
      win[ring<W>(rd + j)] = win[ring<W>(rs + (u32)r)];
    }
    return;
  }
  if (!LINEAR && s >= 0 && dd > W::HIST && rd + l <= W::RW) {
    // wholly in the flushed output (a distance beyond HIST is longer than any match: disjoint): eight octets per lane,
    // one memory round trip for the whole match
    const u32 k = 8 * lane;
    u64 v0 = 0, v1 = 0;
    if (k < l) tbz_gload64x2(S.g0 + s + k, S.g0 + s + k, v0, v1);
    if (k + 8 <= l) {
      k2_st64(win + rd + k, v0);
    } else if (k < l) {
      for (u32 b = 0; b < l - k; b++) win[rd + k + b] = (u8)(v0 >> (8 * b));
    }
    return;
  }
  if (!LINEAR) {
    // octet by octet: each source octet is a pointer (before the group), in the window, or in the flushed output
    for (u32 j0 = 0; j0 < l; j0 += 64) {  // wave-uniform trip count (the loads below are waited for together)
      const u32 j = j0 + lane;
      const bool act = j < l;
      const u32 r = dd >= l ? j : j % dd;
      const i64 t = s + (i64)r;
      u32 b0 = 0, b1 = 0;
      const bool sym = t < 0;
      const bool near = !sym && (i64)gpos - t <= (i64)W::HIST;
      if (act && sym && S.hist) {
        const u32 q = (u32)(32768 + t);  // (a distance is at most 32768)
        b0 = S.plane ? (0x80u | (q >> 8)) : (q & 0xffu);
      } else if (act && near) {
        b0 = win[k2_index<W>(rpos, gpos, t)];
      } else if (act && !sym) {
        tbz_gload8x2(S.g0 + t, S.g0 + t, b0, b1);
      }
      if (act) win[ring<W>(rd + j)] = (u8)b0;
    }
  }
}

// ---- a short match (up to K2_SHORT octets), copied by its own lane.  Whatever their source, its octets travel as A0, A1
// (the first sixteen) and B0, B1 (the last sixteen; up to sixteen octets: B1 alone, the last eight; up to eight: A0 alone).
// The store half: octet-addressed wide LDS accesses, (overlapping) writes that cover exactly [rd, rd + len)
TBZ_DEV void k2_short_store(u8* win, u32 rd, u32 len, u64 A0, u64 A1, u64 B0, u64 B1) {
  if (len >= 17) {
    k2_st64(win + rd, A0);
    k2_st64(win + rd + 8, A1);
    k2_st64(win + rd + len - 16, B0);
    k2_st64(win + rd + len - 8, B1);
  } else if (len >= 9) {
    k2_st64(win + rd, A0);
    k2_st64(win + rd + len - 8, B1);
  } else if (len >= 4) {
    k2_st32(win + rd, (u32)A0);
    k2_st32(win + rd + len - 4, (u32)(A0 >> ((len - 4) * 8)));
  } else {
    k2_st16(win + rd, (u32)A0);
    win[rd + 2] = (u8)(A0 >> 16);
  }
}
// A source inside the window, disjoint from the destination (dist >= len): one or two reads for most matches, then the
// same stores (four 8-octet accesses each way at most: a 16-octet struct copy took a round trip through scratch memory
// here).  Each class loads, then calls the store ladder with a length the compiler knows the class of: after inlining
// the inner ladder folds to that class's stores, so the compiled code walks the length classes once.  (Loading in one
// ladder and storing in a second one — a load half of its own — was measured: every lane takes the divergent branches
// twice per round, K2 13 % slower on the linear and the plain ring groups; profiles/README.md.)
TBZ_DEV void k2_short_copy(u8* win, u32 rs, u32 rd, u32 len) {
  if (len >= 17) {
    const u64 a0 = k2_ld64(win + rs), a1 = k2_ld64(win + rs + 8);
    const u64 b0 = k2_ld64(win + rs + len - 16), b1 = k2_ld64(win + rs + len - 8);
    k2_short_store(win, rd, len, a0, a1, b0, b1);
  } else if (len >= 9) {
    k2_short_store(win, rd, len, k2_ld64(win + rs), 0, 0, k2_ld64(win + rs + len - 8));
  } else if (len >= 4) {
    k2_short_store(win, rd, len, k2_ld64(win + rs), 0, 0, 0);
  } else {
    k2_short_store(win, rd, len, k2_ld32(win + rs), 0, 0, 0);
  }
}
// Octet by octet: overlapping (the match repeats its dist-octet pattern, all of it final already) or at the ring's seam
template <class W>
TBZ_DEV void k2_short_octets(u8* win, u32 rs, u32 rd, u32 len, u32 dist) {
  u32 jj = 0;
  for (u32 j = 0; j < len; j++) {
    win[ring<W>(rd + j)] = win[ring<W>(rs + jj)];
    jj = jj + 1 == dist ? 0 : jj + 1;
  }
}

// RING, round 0: matches whose sources lie outside the window.  far: wholly in the flushed output; symall: wholly before
// the group (computed pointers).  They depend on nothing in flight, so they go first, all at once (one memory round trip
// per batch that has any).  Returns the lanes it settles — with COPY = false it only names them, the copies were another
// wave's — and, in `oddm`, the lanes whose source straddles the group's start (or an invalid stream's distance): those
// are copied one by one in the rounds.
template <class W, bool COPY>
TBZ_DEV u64 k2_far_round(const K2Src& S, u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist, bool mine, u32 rd, i64 s,
                         u64& oddm) {
  constexpr u32 RW = W::RW;
  u8* win = S.win;
  const bool SYM = S.hist != 0;  // (wave-uniform)
  const bool symall = SYM && s + (i64)len <= 0;
  const bool far = !symall && dist > W::HIST && s >= 0;
  const bool odd = mine && !symall && !far && (dist > W::HIST || (SYM && s < 0));
  const bool wide = len <= K2_SHORT && rd + 32 <= RW;
  const u64 farm = tbz_ballot(mine && far), symm = tbz_ballot(mine && symall);
  oddm = tbz_ballot(odd);
  if (!COPY || !(farm | symm)) return farm | symm;
  const bool fw = mine && wide && (far || symall);
  u64 A0 = 0, A1 = 0, B0 = 0, B1 = 0;
  const u64 m17 = tbz_ballot(fw && far && len >= 17);
  if (fw && far) {
    // sixteen octets from the match's first octet for everyone, the last sixteen for the matches longer than that
    // (one load instruction per batch, mostly)
    const u8* p = S.g0 + s;
    tbz_u32x4 L0, L1;
    tbz_gload128x2(p, p + len - 16, m17, L0, L1);
    const u64 lo = ((u64)L0.y << 32) | L0.x, hi = ((u64)L0.w << 32) | L0.z;
    A0 = lo;
    if (len >= 17) {
      A1 = hi;
      B0 = ((u64)L1.y << 32) | L1.x;
      B1 = ((u64)L1.w << 32) | L1.z;
    } else if (len >= 9) {  // octets [len - 8, len) of the sixteen
      const u32 sh = (len - 8) * 8;  // 8 .. 64
      B1 = sh == 64 ? hi : ((lo >> sh) | (hi << (64 - sh)));
    }
  }
  if (fw && symall) {  // computed pointers: the octet plane out of the identity table, the mark plane in arithmetic
    const u32 q = (u32)(32768 + s);
    if (S.plane) {
      A0 = k2_mark8(q);
      if (len >= 9) B1 = k2_mark8(q + len - 8);
      if (len >= 17) {
        A1 = k2_mark8(q + 8);
        B0 = k2_mark8(q + len - 16);
      }
    } else {
      A0 = k2_ld64(S.idt + (q & 255));
      if (len >= 9) B1 = k2_ld64(S.idt + ((q + len - 8) & 255));
      if (len >= 17) {
        A1 = k2_ld64(S.idt + ((q + 8) & 255));
        B0 = k2_ld64(S.idt + ((q + len - 16) & 255));
      }
    }
  }
  if (fw) k2_short_store(win, rd, len, A0, A1, B0, B1);
  // the rest of them (long, or at the ring's seam): one at a time, all lanes
  u64 rest = (farm | symm) & ~tbz_ballot(fw);
  while (rest) {
    const u32 i = (u32)tbz_ffs64(rest) - 1;
    rest &= rest - 1;
    const u32 di = tbz_readlane(dofs, i);
    k2_copy_coop<W>(S, rpos, gpos, (i64)gpos + di, tbz_readlane(rd, i), tbz_readlane(dist, i), tbz_readlane(len, i));
  }
  tbz_sync();
  return farm | symm;
}

// The rounds.  A match is ready when the part of its source that it does not produce itself lies below the high-water
// mark (the offset of the first unresolved match; everything below is final).  The first unresolved match is always
// ready, so every round makes progress.  `oddq` (RING; constant zero for the linear window): matches whose source
// straddles the group's first octet wait their turn like any other (their part inside the group must be final), then
// take the octet-by-octet path.  (The lane's values arrive as plain parameters: a per-lane record passed by reference
// was tried and raised the ring kernels' scalar spills; profiles/README.md.)
template <class W>
TBZ_DEV void k2_rounds(const K2Src& S, u64 pend, u64 oddq, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist, u32 rd, u32 rs, i32 need,
                       bool fastable, u64 longm) {
  constexpr bool LINEAR = W::LINEAR;
  u8* win = S.win;
  const u32 lane = tbz_lane();
  const u64 lane_bit = 1ull << lane;
#ifdef TBZ_WAVE_TRACE
  u32 tr_rounds = 0;
  const u32 tr_matches = (u32)tbz_popc64(pend);
#endif
  while (pend) {
#ifdef TBZ_WAVE_TRACE
    tr_rounds += 1;
#endif
    const u32 first = (u32)tbz_ffs64(pend) - 1;
    if ((oddq >> first) & 1) {  // the first unresolved match is an odd one: everything before it is final
      k2_copy_coop<W>(S, rpos, gpos, (i64)gpos + tbz_readlane(dofs, first), tbz_readlane(rd, first), tbz_readlane(dist, first),
                      tbz_readlane(len, first));
      pend &= pend - 1;
      tbz_sync();
      continue;
    }
    const i32 hwm = (i32)tbz_readlane(dofs, first);
    const bool ready = (pend & lane_bit) && need <= hwm && !((oddq >> lane) & 1);
    const u64 rdy = tbz_ballot(ready);
    u64 longs = rdy & longm;
    if (ready && fastable) {
      k2_short_copy(win, rs, rd, len);
    } else if (ready && len <= K2_SHORT) {
      k2_short_octets<W>(win, rs, rd, len, dist);
    }
    while (longs) {
      const u32 i = (u32)tbz_ffs64(longs) - 1;
      longs &= longs - 1;
      k2_copy_coop<W>(S, rpos, gpos, LINEAR ? 0 : (i64)gpos + tbz_readlane(dofs, i), tbz_readlane(rd, i), tbz_readlane(dist, i),
                      tbz_readlane(len, i));
    }
    pend &= ~rdy;
    tbz_sync();
  }
#ifdef TBZ_WAVE_TRACE
  if (LINEAR && lane == 0 && tr_matches) {
    atomicAdd(&tbz_dbg_cnt[0], 1u);          // batches with matches
    atomicAdd(&tbz_dbg_cnt[1], tr_rounds);   // rounds
    atomicAdd(&tbz_dbg_cnt[2], tr_matches);  // matches
  }
#endif
}

// Multi-round resolution of one batch's matches (at most one per lane).  `pend` = lanes holding an unresolved match;
// dofs = octet offset of the match inside the batch, whose first octet (group-relative offset gpos) sits at window index
// rpos.  RING: k2_far_round first, then k2_rounds over what it left.
// STAGE (ring kernels on three waves, tbz_k2_lz77_ring3): K2_FAR = that first round only, K2_NEAR = everything after it
// (the far round was another wave's, one batch earlier: its memory round trip is off the resolving wave's path).
constexpr u32 K2_ALL = 0, K2_FAR = 1, K2_NEAR = 2;
template <class W, u32 STAGE = K2_ALL>
TBZ_DEV void k2_resolve(const K2Src& S, u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) {
  static_assert(STAGE == K2_ALL || !W::LINEAR, "stages are the ring kernels'");
  constexpr bool LINEAR = W::LINEAR;
  constexpr u32 RW = LINEAR ? 1u : W::RW;
  // this lane's match in window terms, worked out once for the parts below.  mine: the lane holds an unresolved match;
  // rd / rs: window index of its first octet / of its source's (sources inside the window); s: group-relative offset of
  // the source; need: the part of the source the match does not write itself ends at dofs - dist + min(len, dist);
  // fastable: a short disjoint match away from the ring's seam takes the wide accesses
  const bool mine = (pend & (1ull << tbz_lane())) != 0;
  const i32 need = (i32)dofs - (i32)dist + (i32)(len < dist ? len : dist);
  const u32 rd = ring<W>(rpos + dofs);
  const u32 rs = LINEAR ? (rd >= dist ? rd - dist : 0) : (rd >= dist % RW ? rd - dist % RW : rd + RW - dist % RW);
  const u64 longm = tbz_ballot(len > K2_SHORT);
  const bool fastable = len <= K2_SHORT && dist >= len && (LINEAR || (rs + 32 <= RW && rd + 32 <= RW));
  const i64 s = (i64)gpos + dofs - (i64)dist;
  tbz_sync();
  u64 oddq = 0;
  if (!W::LINEAR) {
    u64 oddm;
    pend &= ~k2_far_round<W, STAGE != K2_NEAR>(S, pend, rpos, gpos, dofs, len, dist, mine, rd, s, oddm);
    if (STAGE == K2_FAR) return;
    oddq = oddm & pend;
  }
  k2_rounds<W>(S, pend, oddq, rpos, gpos, dofs, len, dist, rd, rs, need, fastable, longm);
}


// which group this workgroup handles; false: none (beyond the list, or filtered out by size class)
TBZ_DEV bool k2_pick_group(const K2Params& P, u32& gi, Group& g, Seg& sg_guess, u32 at = ~0u) {
  if (at == ~0u) at = tbz_block() + P.first;
  if (at >= P.n_groups) return false;
  gi = P.order ? P.order[at] : at;
  sg_guess = P.segs[gi];  // device-built tables (K3) have segment i in group i: fetched along with the group
  g = P.groups[gi];
  if (!P.order && P.cls) {  // device-built tables (K3): one segment per group, sorted into launches by size here
    const bool small = (g.seg_first == gi ? sg_guess : P.segs[g.seg_first]).out_bytes + K2_SLACK <= K2_SMALL_MAX;
    if ((P.cls == 1) != small) return false;
  }
  return true;
}

// The front end of a group: token fetch, classification, offsets, literals; every batch's matches go to
// `emit(pend, rpos, gpos, dofs, len, dist)` — the resolve step itself in the one-wave kernels, the hand-off to the
// resolving wave in the two-wave kernels — and `finish()` runs before the final flush.
// SPAN: most octets one batch may produce in the ring kernels.  DUAL (ring, two waves): `emit` hands the batch to the
// resolving wave and returns while it is IN FLIGHT — so the ring is flushed only up to that batch's first octet, a
// stored run (which this wave copies into the ring itself) waits for the resolving wave to drain, and the ring must
// hold its history plus TWO spans.
// DUAL = 2 (ring, three waves: front end -> far sources -> resolve): TWO batches are in flight behind the front end.
template <class W, u32 SPAN, u32 DUAL, class Emit, class Finish>
TBZ_DEV void k2_body(const K2Params& P, u32 gi, const Group& g, const Seg& sg_guess, u8* win, u16* tks,
                     u32* rcache, Emit&& emit, Finish&& finish) {
  constexpr bool LINEAR = W::LINEAR;
  static_assert(LINEAR || W::RW >= W::HIST + (DUAL + 1) * SPAN + 64, "ring: history + the spans in flight");
  // what a far match reads has been flushed, and the flush waited for, when its batch is handed over: the flush stops at
  // the oldest batch in flight and happens every K2R_FLUSH octets at the latest
  static_assert(LINEAR || W::HIST >= SPAN + 258 + 16 + (K2R_FLUSH > DUAL * SPAN + 16 ? K2R_FLUSH : DUAL * SPAN + 16),
                "far sources must have been flushed");
  const u32 lane = tbz_lane();
  const u64 lane_bit = 1ull << lane;
  u8* outp = P.out_base + (g.out_abs - P.out_bias);
  const u32 a0 = (u32)((uintptr_t)outp & 15);
  const u64 clip = g.out_end > g.out_abs ? g.out_end - g.out_abs : 0;
  u64 pos = 0, flushed = 0;
  u64 bstart = 0;  // DUAL: first octet of the batch handed over last
  u64 bprev = 0;   // DUAL = 2: ... and of the one before it (everything before the OLDEST batch in flight is resolved)
  u32 rpos = a0;   // window index of `pos`
  const u32 litmask = (!LINEAR && P.plane) ? 0u : 0xffu;  // mark plane: every octet this group produces itself is "known" = 0
  bool stores_in_flight = false;  // RING: a flush has been issued since the last wait (a far match reads what it stored)
  auto flush_upto = [&](u64 upto) {
    if (upto <= flushed) return;
    k2_flush<W>(win, outp, flushed, upto, clip, a0);
    flushed = upto;
    stores_in_flight = true;
  };
  auto emit_batch = [&](u64 pend, u32 dofs, u32 len, u32 dist) {
    bprev = bstart;
    bstart = pos;
    if (!LINEAR && stores_in_flight) {  // (wave-uniform) what was flushed must have arrived before a resolve step reads it back
      tbz_vm_drain();
      stores_in_flight = false;
    }
    emit(pend, rpos, pos, dofs, len, dist);
  };

  for (u32 s = 0; s < g.seg_count && pos < clip; s++) {
    const Seg sg = g.seg_first + s == gi ? sg_guess : P.segs[g.seg_first + s];
    u64 p = 0;
    // The segment's token stream is the concatenation of its runs (8-word pieces).  Token ring: chunk c
    // (logical words [c*K2_TCH, (c+1)*K2_TCH) = 64 pieces, one per lane) lives in ring half c & 1.  The
    // chunk after the one in use is already on its way in registers, so a batch never waits on memory
    // except at the start of a segment.  A cache of 64 run records (inclusive piece counts rE, offsets rO,
    // in LDS) maps logical pieces to addresses; it is re-based when a chunk reaches past it.
    const u64 npieces = sg.tok_words >> 3;
    // (a repaired segment's tokens live in the repair launches' own pool: a gang that repairs runs past the
    // marker it will land on, and must not scribble over the tokens of the items that start there)
    const RunRec* rt = (const RunRec*)sg.runs + sg.run_first;  // (the item's run 0 lives in the segment record)
    const u16* tbase = (const u16*)sg.tok;                     // run offsets count 8-word granules from here
    u32* rE = rcache;
    u32* rO = rcache + 64;
    u32 rbase = 0, ctot = 0;
    u64 cbase = 0;
    auto load_cache = [&]() {
      RunRec rr{};
      if (rbase + lane < sg.n_runs) rr = (sg.run_first + rbase + lane) ? rt[rbase + lane] : sg.run0;
      const u32 inc = tbz_wave_incl_scan_u32(rr.n8);
      tbz_sync();
      rE[lane] = inc;
      rO[lane] = rr.off8;
      tbz_sync();
      ctot = tbz_shfl(inc, 63);
    };
    auto find_run = [&](u32 rel) -> u32 {  // first cached run whose inclusive end is beyond piece `rel`
      u32 j = 0;
#pragma unroll
      for (u32 step = 32; step; step >>= 1) j += rE[j + step - 1] <= rel ? step : 0u;
      return j;
    };
    // the same for the 64 pieces of one chunk, whose first piece lies in run j0: a chunk usually spans two or
    // three runs, so four broadcast reads answer it; the binary search is the fallback
    auto find_run_from = [&](u32 j0, u32 rel) -> u32 {
      const u32 e0 = rE[j0], e1 = rE[j0 + 1 < 64 ? j0 + 1 : 63], e2 = rE[j0 + 2 < 64 ? j0 + 2 : 63], e3 = rE[j0 + 3 < 64 ? j0 + 3 : 63];
      const u32 j = j0 + (rel >= e0 ? 1u : 0u) + (rel >= e1 ? 1u : 0u) + (rel >= e2 ? 1u : 0u);
      return (rel < e3 && j0 + 3 < 64) ? j : find_run(rel);
    };
    u32 jn = 0;  // cached run that holds the first piece of the next chunk (chunks are fetched in order)
    auto cover = [&](u64 x0, u64 xl) {  // make the cache hold pieces x0..xl (a chunk: at most 64 pieces)
      if (xl - cbase < ctot) return;
      if (x0 - cbase < ctot) {
        cbase += jn ? rE[jn - 1] : 0u;
        rbase += jn;
      } else {
        cbase += ctot;
        rbase += 64;
      }
      jn = 0;
      load_cache();
    };
    auto fetch = [&](u32 c) -> uint4 {  // this lane's piece of chunk c
      uint4 v{};
      const u64 x0 = (u64)c * 64;
      if (x0 >= npieces) return v;
      const u64 xl = x0 + 63 < npieces ? x0 + 63 : npieces - 1;
      cover(x0, xl);
      const u64 x = x0 + lane;
      u32 j = jn;
      if (x < npieces) {
        const u32 rel = (u32)(x - cbase);
        j = find_run_from(jn, rel);
        const u32 before = j ? rE[j - 1] : 0u;
        v = *(const uint4*)(tbase + ((u64)rO[j] + (rel - before)) * 8);
      }
      const u32 jl = tbz_readlane(j, (u32)(xl - x0));  // the run of the chunk's last piece
      jn = jl + ((u32)(xl - cbase) + 1 >= rE[jl] ? 1u : 0u);
      return v;
    };
    u32 cur = 0;
    load_cache();
    const uint4 v0 = fetch(0);
    uint4 pre = fetch(1);
    tbz_sync();
    *(uint4*)(tks + lane * 8) = v0;
    tbz_sync();
    while (p < sg.tok_words && pos < clip) {
      const u64 left = sg.tok_words - p;
      const u32 n2 = left < 128 ? (u32)left : 128;
      if ((p + n2 - 1) / K2_TCH > cur) {  // the batch reaches into the next chunk: land it, fetch the one after
        cur += 1;
        tbz_sync();
        *(uint4*)(tks + (cur & 1) * K2_TCH + lane * 8) = pre;
        pre = fetch(cur + 1);
        tbz_sync();
      }
      // ---- two words per lane: words 2*lane and 2*lane+1 of the batch
      const bool va = 2 * lane < n2, vb = 2 * lane + 1 < n2;
      const u32 a = va ? tks[((u32)p + 2 * lane) & (K2_TOKBUF - 1)] : 0;
      const u32 b = vb ? tks[((u32)p + 2 * lane + 1) & (K2_TOKBUF - 1)] : 0;
      if (tbz_ballot((a & 0xC000u) == 0xC000u || (b & 0xC000u) == 0xC000u) == 0) {
        // ---- no stored run in sight.  A word with bit 15 set is a match head and the word after it its
        // distance (bit 15 clear), so heads need no context; a lane holds at most one match.
        const bool ha = (a & 0x8000u) != 0, hb = (b & 0x8000u) != 0;
        const bool hav = ha && vb;                 // head with its distance word inside the batch
        const bool hbv = hb && 2 * lane + 2 < n2;
        const bool pa = tbz_wave_shr1(hb ? 1u : 0u) != 0;  // word a is the previous lane's distance word
        const bool la = va && !ha && !pa && !(a & TOK_NOP), lb = vb && !hb && !ha && !(b & TOK_NOP);  // no-ops count for nothing
        const u32 len_a = hav ? (a & 0xff) + 3 : (la ? 1u : 0u);
        const u32 len_b = hbv ? (b & 0xff) + 3 : (lb ? 1u : 0u);
        const u32 sum = len_a + len_b;
        const u32 incl = tbz_wave_incl_scan_u32(sum);
        // words this lane accounts for: its own (0..2) plus, for a head in word b, the distance word after
        const u32 cw = (ha && !vb) ? 0u : !vb ? 1u : (hb && !hbv) ? 1u : hbv ? 3u : 2u;
        u32 nl = (n2 + 1) >> 1;  // lanes holding words
        if (!LINEAR) {           // the ring must not be overrun inside one batch
          const u64 over = tbz_ballot(incl > SPAN);
          const u32 lok = over ? (u32)tbz_ffs64(over) - 1 : 64u;
          nl = nl < lok ? nl : lok;
        }
        const u32 last = nl - 1;  // nl >= 1: one lane produces at most 259 octets
        const u32 m = 2 * last + tbz_readlane(cw, last);
        if (m == 0) break;  // malformed token stream (never produced by K1)
        const u32 total = tbz_readlane(incl, last);
        const bool act = lane <= last;
        const u32 oa = incl - sum, ob = oa + len_a;
        if (la && act) win[ring<W>(rpos + oa)] = (u8)(a & litmask);
        if (lb && act) win[ring<W>(rpos + ob)] = (u8)(b & litmask);
        const u32 na = tbz_wave_shl1(a);  // next lane's word a: the distance word of a head in b
        const bool hasm = (hav || hbv) && act;
        const u32 len = hav ? len_a : len_b;
        const u32 dist = ((hav ? b : na) & 0x7fffu) + 1;
        emit_batch(tbz_ballot(hasm), hav ? oa : ob, hasm ? len : 0u, dist);
        pos += total;
        rpos = ring<W>(rpos + total);
        p += m;
      } else {
        // ---- a stored run within reach: one word per lane, up to the run (or the run itself)
        const u32 n = left < 64 ? (u32)left : 64;
        const u32 w = lane < n ? tks[((u32)p + lane) & (K2_TOKBUF - 1)] : 0;
        const u64 valid = n == 64 ? ~0ull : ((1ull << n) - 1);
        u64 hbm = tbz_ballot((w & 0x8000u) != 0) & valid;        // heads (payload words have bit 15 clear)
        u64 sb = tbz_ballot((w & 0xC000u) == 0xC000u) & valid;   // stored-run heads
        u64 mb = hbm & ~sb;                                      // match heads
        if (sb & 1) {
          // stored run at the front of the batch: cooperative copy input -> window, flushing as we go
          if (n < 4) break;  // malformed (never produced by K1)
          u32 w1 = tbz_readlane(w, 1), w2 = tbz_readlane(w, 2), w3 = tbz_readlane(w, 3), w0 = tbz_readlane(w, 0);
          u64 cnt = (w0 & 0x3fff) | ((u64)(w1 & 3) << 14);
          u64 src = ((u64)(w1 >> 2) & 0x1fff) | ((u64)w2 << 13) | ((u64)w3 << 28);
          // an empty batch per batch in flight: when their hand-overs have returned, everything before is resolved
          for (u32 e = 0; e < DUAL; e++) emit_batch(0ull, 0u, 0u, 1u);
          while (cnt) {
            u32 c = cnt < SPAN ? (u32)cnt : SPAN;  // (the ring holds its history + one span)
            tbz_sync();
            // eight octets per lane and trip (octet-addressed accesses on both sides); octet by octet at the chunk's end
            // and across the ring's seam
            for (u32 j = lane * 8; j < c; j += 512) {
              const u32 r = ring<W>(rpos + j);
              if (j + 8 <= c && (LINEAR || r + 8 <= W::RW)) {
                k2_st64(win + r, litmask ? k2_ld64(P.in_base + src + j) : 0ull);
              } else {
                for (u32 k = 0; k < 8 && j + k < c; k++) win[ring<W>(rpos + j + k)] = (u8)(P.in_base[src + j + k] & litmask);
              }
            }
            tbz_sync();
            pos += c;
            rpos = ring<W>(rpos + c);
            src += c;
            cnt -= c;
            bstart = bprev = pos;
            if (!LINEAR && (pos - flushed >= K2R_FLUSH || pos >= clip))
              flush_upto(pos >= clip ? pos : ((pos + a0) & ~15ull) - a0);
            if (pos >= clip) break;
          }
          p += 4;
          continue;
        }
        // everything before the first stored head
        u32 n_eff = sb ? (u32)tbz_ffs64(sb) - 1 : n;
        const u64 veff = n_eff == 64 ? ~0ull : ((1ull << n_eff) - 1);
        mb &= veff;
        u64 pm = (mb << 1);               // payload (distance) words
        u64 nops = tbz_ballot((w & 0xC000u) == TOK_NOP) & veff & ~pm;
        u64 lits = veff & ~mb & ~pm & ~nops;
        u64 cut_ok = (lits | pm | nops) & veff;  // a batch may end after a literal, a no-op or a distance word
        bool head = (mb & lane_bit) != 0, islit = (lits & lane_bit) != 0;
        u32 len = head ? (w & 0xff) + 3 : (islit ? 1u : 0u);
        u32 incl = tbz_wave_incl_scan_u32(len);
        u64 ok = LINEAR ? cut_ok : (tbz_ballot(incl <= SPAN) & cut_ok);
        if (ok == 0) break;  // malformed token stream (never produced by K1)
        u32 m = 64 - (u32)__builtin_clzll(ok);
        u32 total = tbz_readlane(incl, m - 1);
        const u64 act = m == 64 ? ~0ull : ((1ull << m) - 1);
        u32 dofs = incl - len;  // octet offset of this token inside the batch
        u32 dist = (tbz_wave_shl1(w) & 0x7fffu) + 1;
        if (islit && (act & lane_bit)) win[ring<W>(rpos + dofs)] = (u8)(w & litmask);
        emit_batch(mb & act, dofs, len, dist);
        pos += total;
        rpos = ring<W>(rpos + total);
        p += m;
      }
      if (!LINEAR && pos - flushed >= K2R_FLUSH) {
        const u64 lim = DUAL == 2 ? bprev : DUAL ? bstart : pos;
        const u64 al = (lim + a0) & ~15ull;  // keep the unaligned tail in the ring
        // (al <= a0: nothing is final yet — a FIRST batch of K2R_FLUSH octets or more, which only a flush interval at or
        // below the batch span allows; such a build flushed the whole group from an empty ring: found on config 5)
        if (al > a0) flush_upto(al - a0);
      }
    }
  }
  finish(pos < clip ? pos : clip, a0);
  k2_flush<W>(win, outp, flushed, pos, clip, a0);
}

// ring launches: which group, and which plane of it, this workgroup decodes (Q = the launch parameters as k2_body wants
// them for that group)
TBZ_DEV bool k2_ring_select(const K2Params& P, K2Params& Q, u32& gi, Group& g, Seg& sg_guess) {
  Q = P;
  if (!P.mixed) return k2_pick_group(P, gi, g, sg_guess);
  const u32 b = tbz_block();
  u32 at = b;
  if (b >= P.n_plain) {
    const u32 h = b - P.n_plain;
    at = P.n_plain + (h >> 1);
    Q.hist = 1;
    Q.plane = h & 1;
    if (h & 1) {
      Q.out_base = P.mark_base;
      Q.out_bias = P.mark_bias;
    }
  }
  return k2_pick_group(P, gi, g, sg_guess, at);
}
// identity octets (the octet plane of computed pointers)
TBZ_DEV void k2_idt_init(u8* idt, u32 nthreads) {
  for (u32 k = tbz_lane() + 64 * tbz_wave(); k < K2_IDT; k += nthreads) idt[k] = (u8)k;
}

// ---- the ring kernel on ONE wave (TBZ_K2_MODE=single): front end and resolve in turn
TBZ_KERNEL void tbz_k2_lz77(K2Params P) {
  TBZ_SHARED __attribute__((aligned(16))) u8 win[K2R_RW];
  TBZ_SHARED __attribute__((aligned(16))) u8 idt[K2_IDT];
  TBZ_SHARED __attribute__((aligned(16))) u16 tks[K2_TOKBUF];
  TBZ_SHARED u32 rcache[128];
  u32 gi;
  Group g;
  Seg sg;
  K2Params Q;
  if (!k2_ring_select(P, Q, gi, g, sg)) return;
  k2_idt_init(idt, 64);
  tbz_sync();
  K2Src S{win, idt, Q.out_base + (g.out_abs - Q.out_bias), Q.hist, Q.plane};
  k2_body<K2Ring, K2_SPAN, false>(
      Q, gi, g, sg, win, tks, rcache,
      [&](u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) { k2_resolve<K2Ring>(S, pend, rpos, gpos, dofs, len, dist); },
      [](u64, u32) {});
}

// groups whose output (plus K2_SLACK octets) fits P.win_bytes, one wave doing everything
TBZ_KERNEL void tbz_k2_lz77_small(K2Params P) {
  TBZ_DYN_SHARED(u8, dyn);
  u32 gi;
  Group g;
  Seg sg;
  if (!k2_pick_group(P, gi, g, sg)) return;
  u8* win = dyn;
  K2Src S{win, nullptr, nullptr, 0, 0};
  k2_body<K2Linear, K2L_SPAN, false>(
      P, gi, g, sg, win, (u16*)(dyn + P.win_bytes), (u32*)(dyn + P.win_bytes + 2 * K2_TOKBUF),
      [&](u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) { k2_resolve<K2Linear>(S, pend, rpos, gpos, dofs, len, dist); },
      [](u64, u32) {});
}

// The same groups with TWO wavefronts per workgroup over one window: wave 0 runs the front end of batch k
// (token fetch, classification, prefix sum, literals) while wave 1 resolves the matches of batch k-1; they
// meet at a workgroup barrier once per batch and hand the match descriptors over through LDS.  Both halves
// are latency-bound chains, so overlapping them (and doubling the waves per CU at the same LDS) is what pays.
// Safe because a batch's front end only writes octets at or beyond its own start (literals, stored runs),
// which the resolve of the previous batch neither reads as a source nor writes.
struct K2Hand {
  u64 desc[64];  // per lane: dofs | len << 16 | dist << 32
  u64 pend;      // lanes holding a match
  u64 gpos;      // group-relative offset of the batch's first octet
  u32 rpos;      // window index of the batch's first octet
  u32 end;       // 1: no batch — the group is done
};
TBZ_KERNEL_WG(128, 2) void tbz_k2_lz77_dual(K2Params P) {
  TBZ_DYN_SHARED(u8, dyn);
  u32 gi;
  Group g;
  Seg sg;
  if (!k2_pick_group(P, gi, g, sg)) return;  // both waves take the same decision
  const u32 lane = tbz_lane();
  u8* win = dyn;
  K2Hand* H = (K2Hand*)(dyn + P.win_bytes + 2 * K2_TOKBUF + 512);
  [[maybe_unused]] const u64 tr0 = TBZ_TR_NOW();
  [[maybe_unused]] u64 tr_wait = 0, tr_x = 0;
  if (tbz_wave() == 0) {
    u32 k = 0;
    k2_body<K2Linear, K2L_SPAN, false>(
        P, gi, g, sg, win, (u16*)(dyn + P.win_bytes), (u32*)(dyn + P.win_bytes + 2 * K2_TOKBUF),
        [&](u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) {
          K2Hand& h = H[k & 1];
          h.desc[lane] = (u64)dofs | ((u64)len << 16) | ((u64)dist << 32);
          if (lane == 0) {
            h.pend = pend;
            h.rpos = rpos;
            h.gpos = gpos;
            h.end = 0;
          }
          tr_x = TBZ_TR_NOW();
          tbz_wg_barrier();
          tr_wait += TBZ_TR_NOW() - tr_x;
          k += 1;
        },
        [&](u64 n_out, u32 a0) {
          if (lane == 0) {
            K2Hand& h = H[k & 1];
            h.end = 1;
            h.pend = n_out;  // what wave 1 needs for the checksum: octets of the group, window index of the first
            h.rpos = a0;
          }
          tr_x = TBZ_TR_NOW();
          tbz_wg_barrier();
          tr_wait += TBZ_TR_NOW() - tr_x;
#ifdef TBZ_WAVE_TRACE
          if (lane == 0 && tbz_block() < 8192) {
            tbz_dbg[tbz_block() * 8 + 0] = tr0;
            tbz_dbg[tbz_block() * 8 + 2] = tr_wait;
            tbz_dbg[tbz_block() * 8 + 3] = k;
            tbz_dbg[tbz_block() * 8 + 6] = TBZ_TR_NOW();
          }
#endif
        });
#ifdef TBZ_WAVE_TRACE
    if (lane == 0 && tbz_block() < 8192) tbz_dbg[tbz_block() * 8 + 1] = TBZ_TR_NOW();
#endif
  } else {
    K2Src S{win, nullptr, nullptr, 0, 0};
    for (u32 k = 0;; k++) {
      if (k > 0) {
        const K2Hand& h = H[(k - 1) & 1];
        const u64 d = h.desc[lane];
        k2_resolve<K2Linear>(S, h.pend, h.rpos, h.gpos, (u32)(d & 0xffffu), (u32)((d >> 16) & 0xffffu), (u32)(d >> 32));
      }
      tr_x = TBZ_TR_NOW();
      tbz_wg_barrier();
      tr_wait += TBZ_TR_NOW() - tr_x;
      if (H[k & 1].end) {
        // every match is resolved: while wave 0 flushes the window, this wave takes the group's adler32
        // partial from it (A = sum b_i, B = sum (n - i) b_i; checksums.lisp:18-62 split for the combine)
        if (P.gck) {
          const u32 n = (u32)H[k & 1].pend;
          const u8* w = win + H[k & 1].rpos;
          u64 A = 0, B = 0;
          for (u32 c = lane * 16; c < n; c += 64 * 16) {
            const K2U128 v = *(const K2U128*)(w + c);  // the window is K2_SLACK longer than the output: reads stay inside
            u32 d[4] = {(u32)v.lo, (u32)(v.lo >> 32), (u32)v.hi, (u32)(v.hi >> 32)};
            if (n - c < 16) {  // the group's last, partial piece: octets past the end count for nothing
              const u32 lim = n - c;
#pragma unroll
              for (u32 q = 0; q < 4; q++) {
                const u32 valid = lim > 4 * q ? (lim - 4 * q < 4 ? lim - 4 * q : 4u) : 0u;
                d[q] &= valid == 4 ? ~0u : ((1u << (8 * valid)) - 1);
              }
            }
            u32 a16 = tbz_sum4_u8(d[0], 0);
            a16 = tbz_sum4_u8(d[1], a16);
            a16 = tbz_sum4_u8(d[2], a16);
            a16 = tbz_sum4_u8(d[3], a16);
            u32 w16 = tbz_dot4_u8(d[0], 0x03020100u, 0);
            w16 = tbz_dot4_u8(d[1], 0x07060504u, w16);
            w16 = tbz_dot4_u8(d[2], 0x0b0a0908u, w16);
            w16 = tbz_dot4_u8(d[3], 0x0f0e0d0cu, w16);
            A += a16;
            B += (u64)(n - c) * a16 - w16;
          }
          A = wave_sum_u64(A);
          B = wave_sum_u64(B % ADLER_P);
          if (lane == 0) {
            CkPartial r;
            r.a = (u32)(A % ADLER_P);
            r.b = (u32)(B % ADLER_P);
            P.gck[gi] = r;
            CkChunk ch;
            ch.out_abs = g.out_abs;
            ch.len = n;
            ch.stream = 0;
            P.gchunks[gi] = ch;
          }
        }
        break;
      }
    }
#ifdef TBZ_WAVE_TRACE
    if (lane == 0 && tbz_block() < 8192) {
      tbz_dbg[tbz_block() * 8 + 4] = tr_wait;
      tbz_dbg[tbz_block() * 8 + 5] = TBZ_TR_NOW();
    }
#endif
  }
}

// The ring kernel on TWO wavefronts (front end || resolve, as tbz_k2_lz77_dual does for the linear window): groups
// larger than a linear window, and H-groups (one workgroup per plane).  A batch produces at most K2R_SPAN octets, so
// that the batch in flight and the one the front end is writing both fit beside the history.  15.3 KB of LDS: ten
// workgroups per CU.
TBZ_KERNEL_WG(128, 5) void tbz_k2_lz77_ring2(K2Params P) {
  TBZ_SHARED __attribute__((aligned(16))) u8 win[K2R_RW];
  TBZ_SHARED __attribute__((aligned(16))) u8 idt[K2_IDT];
  TBZ_SHARED __attribute__((aligned(16))) u16 tks[K2_TOKBUF];
  TBZ_SHARED u32 rcache[128];
  TBZ_SHARED K2Hand H[2];
  u32 gi;
  Group g;
  Seg sg;
  K2Params Q;
  if (!k2_ring_select(P, Q, gi, g, sg)) return;  // both waves take the same decision
  const u32 lane = tbz_lane();
  k2_idt_init(idt, 128);
  tbz_wg_barrier();
  if (tbz_wave() == 0) {
    u32 k = 0;
    k2_body<K2Ring, K2R_SPAN, true>(
        Q, gi, g, sg, win, tks, rcache,
        [&](u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) {
          K2Hand& h = H[k & 1];
          h.desc[lane] = (u64)dofs | ((u64)len << 16) | ((u64)dist << 32);
          if (lane == 0) {
            h.pend = pend;
            h.rpos = rpos;
            h.gpos = gpos;
            h.end = 0;
          }
          tbz_wg_barrier();
          k += 1;
        },
        [&](u64, u32) {
          if (lane == 0) H[k & 1].end = 1;
          tbz_wg_barrier();  // the last batch is resolved when this returns: the final flush may read the window
        });
  } else {
    K2Src S{win, idt, Q.out_base + (g.out_abs - Q.out_bias), Q.hist, Q.plane};
    for (u32 k = 0;; k++) {
      if (k > 0) {
        const K2Hand& h = H[(k - 1) & 1];
        const u64 d = h.desc[lane];
        k2_resolve<K2Ring>(S, h.pend, h.rpos, h.gpos, (u32)(d & 0xffffu), (u32)((d >> 16) & 0xffffu), (u32)(d >> 32));
      }
      tbz_wg_barrier();
      if (H[k & 1].end) break;
    }
  }
}

// The ring kernel on THREE wavefronts: front end -> far sources -> resolve, a batch moving one stage per workgroup
// barrier.  What a batch copies from the flushed output (distances beyond the ring's history) or out of computed
// pointers depends on nothing in flight, so the middle wave lands it in the ring while the batch before is still being
// resolved: the memory round trip of the far round — a third of a batch's resolve time — leaves the critical path.  The
// ring holds its history and THREE spans; the front end flushes up to the oldest batch in flight.  H[j % 3] = batch j.
constexpr u32 K2R3_RW = K2R_HIST + 3 * K2R_SPAN + 64;
static_assert(K2R3_RW % 16 == 0, "16-octet chunks must not straddle the ring's seam");
using K2Ring3 = K2W<K2R3_RW, K2R_HIST>;
TBZ_KERNEL_WG(192, 6) void tbz_k2_lz77_ring3(K2Params P) {
  TBZ_SHARED __attribute__((aligned(16))) u8 win[K2R3_RW];
  TBZ_SHARED __attribute__((aligned(16))) u8 idt[K2_IDT];
  TBZ_SHARED __attribute__((aligned(16))) u16 tks[K2_TOKBUF];
  TBZ_SHARED u32 rcache[128];
  TBZ_SHARED K2Hand H[3];
  u32 gi;
  Group g;
  Seg sg;
  K2Params Q;
  if (!k2_ring_select(P, Q, gi, g, sg)) return;  // all three waves take the same decision
  const u32 lane = tbz_lane();
  const u32 wv = tbz_wave();
  k2_idt_init(idt, 192);
  tbz_wg_barrier();
  if (wv == 0) {
    u32 k = 0;
    k2_body<K2Ring3, K2R_SPAN, 2>(
        Q, gi, g, sg, win, tks, rcache,
        [&](u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) {
          K2Hand& h = H[k % 3];
          h.desc[lane] = (u64)dofs | ((u64)len << 16) | ((u64)dist << 32);
          if (lane == 0) {
            h.pend = pend;
            h.rpos = rpos;
            h.gpos = gpos;
            h.end = 0;
          }
          tbz_wg_barrier();
          k += 1;
        },
        [&](u64, u32) {
          if (lane == 0) H[k % 3].end = 1;
          tbz_wg_barrier();  // the last batch has its far sources ...
          tbz_wg_barrier();  // ... and is resolved: the final flush may read the window
        });
  } else {
    K2Src S{win, idt, Q.out_base + (g.out_abs - Q.out_bias), Q.hist, Q.plane};
    for (u32 k = 0;; k++) {
      tbz_wg_barrier();  // batch k has been handed over
      const bool end = H[k % 3].end != 0;
      // wave 1: the far round of batch k; wave 2: the rest of batch k - 1
      const u32 j = wv == 1 ? k : k - 1;
      if ((wv == 1 && !end) || (wv == 2 && k > 0)) {
        const K2Hand& h = H[j % 3];
        const u64 d = h.desc[lane];
        const u32 dofs = (u32)(d & 0xffffu), len = (u32)((d >> 16) & 0xffffu), dist = (u32)(d >> 32);
        if (wv == 1) k2_resolve<K2Ring3, K2_FAR>(S, h.pend, h.rpos, h.gpos, dofs, len, dist);
        else k2_resolve<K2Ring3, K2_NEAR>(S, h.pend, h.rpos, h.gpos, dofs, len, dist);
      }
      if (end) {
        tbz_wg_barrier();
        break;
      }
    }
  }
}

// ================================================================================================
// K6 — LZ77 references across groups (replaces the sequential dependency of copy-history on
// everything before it, deflate.lisp:343-352, for groups decoded in parallel).
//
// A group that needs history it does not hold (an "H-group": its matches reach before its first octet, and the
// groups before it are decoded by other workgroups at the same time) runs through the ring kernel twice — K2's
// copies are the same whatever the octets are — against a window whose first 32 KiB hold POINTERS (see k2_body):
//   plane 0 -> out:  the octet, or the low octet of a pointer
//   plane 1 -> mark: 0, or 0x80 | the pointer's high bits
// so after K2 every octet of an H-group is either final or "octet i of the 32 KiB before this group".  What later
// groups can see of a group is its last 32 KiB (its TAIL), so the dependent chain runs over tails only:
//   1. tbz_k6_chain_sym   blocks of consecutive H-groups, all blocks in parallel: one workgroup walks its block's
//                         tails in order through a 32 KiB ring of SYMBOLS and rewrites them relative to the 32 KiB
//                         before the BLOCK (pointers of pointers collapse);
//   1b. tbz_k6_chain_sym  again, one level up: superblocks of consecutive blocks; a workgroup walks the last 32 KiB of
//                         its superblock's blocks and rewrites them relative to the 32 KiB before the SUPERBLOCK;
//   2. tbz_k6_chain       one workgroup per stream walks the superblocks in order and makes each one's last 32 KiB
//                         final out of a ring of final octets;
//   3. tbz_k6_resolve     everything else in parallel, its sources being final by then: the blocks' last 32 KiB
//                         (relative to their superblock), then the other tail octets (relative to their block), then
//                         every H-group's octets before its tail (relative to itself).
// The chain is three times the cube root of the number of H-groups instead of one step per group (the host sizes
// blocks and superblocks: tbz_engine.hpp); a step is one LDS gather round, workgroup barriers and the stores.
// ================================================================================================
struct K6Range {   // the symbolic octets of [lo, hi): pointer i stands for the octet at absolute offset base - 32768 + i
  u64 base, lo, hi;
  u64 floor;       // the stream's first octet (no pointer reaches below it in a valid stream)
};
struct K6List {
  u32 first, count;  // ranges [first, first+count), walked in order by one workgroup
};
struct K6Params {
  u8* out_base;
  u8* mark_base;     // mark plane: octet x of the output has its mark at mark_base[x - bias]
  u64 bias;
  const K6Range* ranges;
  const K6List* lists;
  u32 n_ranges, n_lists;
  u32 pieces;        // tbz_k6_resolve: workgroups per range (K6_PIECE octets each)
};
constexpr u32 K6_THREADS = 1024;
constexpr u32 K6_PIECE = 4096;
constexpr u32 K6_W = 32768;

// per-octet masks over a dword: 0xff where the mark octet says "symbolic" (bit 7), and where the octet's absolute
// offset x + k lies inside [lo, hi)
TBZ_DEV u32 k6_marked(u32 mw) { return ((mw >> 7) & 0x01010101u) * 0xffu; }
TBZ_DEV u32 k6_inrange(u64 x, u64 lo, u64 hi) {
  u32 r = 0;
#pragma unroll
  for (u32 k = 0; k < 4; k++) r |= ((i64)(x + k) >= (i64)lo && (i64)(x + k) < (i64)hi) ? 0xffu << (8 * k) : 0u;
  return r;
}
// One thread's chunk: the 16 octets at absolute offsets [x, x+16) (x 16-aligned in ADDRESS space), planes o / m.
// Every symbolic octet (inside [lo, hi) unless WHOLE says the chunk lies inside anyway) is replaced by what its
// pointer refers to: src(i, a, b) yields the source's two planes.  All sixteen lookups go out together, symbolic or
// not, and the result is merged in with masks: straight-line code.  Returns whether anything was replaced.
template <bool WHOLE, class Src>
TBZ_DEV bool k6_fix16(uint4& o, uint4& m, u64 x, u64 lo, u64 hi, Src&& src) {
  if ((m.x | m.y | m.z | m.w) == 0) return false;
  u32 ow[4] = {o.x, o.y, o.z, o.w}, mw[4] = {m.x, m.y, m.z, m.w};
  u32 n0[4] = {0, 0, 0, 0}, n1[4] = {0, 0, 0, 0};
#pragma unroll
  for (u32 q = 0; q < 16; q++) {
    const u32 sh = 8 * (q & 3);
    const u32 mb = tbz_bfe(mw[q >> 2], sh, 7), ob = tbz_bfe(ow[q >> 2], sh, 8);
    u32 a, b;
    src((mb << 8) | ob, a, b);
    n0[q >> 2] |= a << sh;
    n1[q >> 2] |= b << sh;
  }
  u32 any = 0;
#pragma unroll
  for (u32 k = 0; k < 4; k++) {
    u32 bm = k6_marked(mw[k]);
    if (!WHOLE) bm &= k6_inrange(x + 4 * k, lo, hi);
    ow[k] = (ow[k] & ~bm) | (n0[k] & bm);
    mw[k] = (mw[k] & ~bm) | (n1[k] & bm);
    any |= bm;
  }
  o = uint4{ow[0], ow[1], ow[2], ow[3]};
  m = uint4{mw[0], mw[1], mw[2], mw[3]};
  return any != 0;
}

struct K6R {  // a K6Range in wave-uniform registers
  u64 base, lo, hi, floor;
};
TBZ_DEV K6R k6_range(const K6Params& P, u32 i) {
  const u64* q = (const u64*)(P.ranges + i);
  K6R r;
  r.base = tbz_uniform64(q[0]);
  r.lo = tbz_uniform64(q[1]);
  r.hi = tbz_uniform64(q[2]);
  r.floor = tbz_uniform64(q[3]);
  return r;
}

// SYM = false: the ring holds FINAL octets; every range comes out final (marks cleared).
// SYM = true:  the ring holds SYMBOLS relative to the list's first base B0 (ring octets of [B0-32768, B0) start out as
//              the identity pointers); ranges come out relative to B0.  The ranges of a list are then the tails of
//              CONSECUTIVE groups (range r+1's base is range r's hi), which the host guarantees.
// A range is at most 32 KiB (+ alignment): two 16-octet chunks per thread, and a third for thread 0.
template <bool SYM>
TBZ_DEV void k6_chain(const K6Params& P, u8* W0, u8* W1) {
  const u32 tid = tbz_wave() * 64 + tbz_lane();
  if (tbz_block() >= P.n_lists) return;
  const u32 first = tbz_uniform(P.lists[tbz_block()].first), count = tbz_uniform(P.lists[tbz_block()].count);
  if (count == 0) return;
  const uintptr_t ob = (uintptr_t)P.out_base;
  // the octet at absolute offset x sits at ring index (address of x) & 32767: chunks that are 16-octet aligned in
  // memory are aligned in the ring too
  u64 w_lo = 0, w_hi = 0;  // the ring holds [w_lo, w_hi)
  K6R g = k6_range(P, first);
  if (SYM) {
    const u64 B0 = g.base;
    for (u32 i = tid * 4; i < K6_W; i += K6_THREADS * 4) {
      const u64 x = B0 - K6_W + i;
#pragma unroll
      for (u32 q = 0; q < 4; q++) {
        const u32 r = (u32)((ob + x + q) & (K6_W - 1));
        W0[r] = (u8)(i + q);
        W1[r] = (u8)(0x80u | ((i + q) >> 8));
      }
    }
    w_lo = B0 - K6_W;
    w_hi = B0;
  }
  // a range's planes do not depend on the chain (K2 wrote them): they are fetched one step ahead — and its record two
  // steps ahead — so that a step is LDS gathers, two barriers and the stores
  uint4 o0{}, o1{}, o2{}, m0{}, m1{}, m2{};
  auto chunk_x = [&](const K6R& r, u32 k) { return (r.lo - ((ob + r.lo) & 15)) + ((u64)tid + (u64)k * K6_THREADS) * 16; };
  auto fetch = [&](const K6R& r, u32 k, uint4& o, uint4& m) {
    const u64 x = chunk_x(r, k);
    if (r.hi > r.lo && (i64)x < (i64)r.hi) {
      o = *(const uint4*)(P.out_base + x);
      m = *(const uint4*)(P.mark_base + (x - P.bias));
    }
  };
  fetch(g, 0, o0, m0);
  fetch(g, 1, o1, m1);
  if (tid == 0) fetch(g, 2, o2, m2);
  K6R gn = count > 1 ? k6_range(P, first + 1) : g;
  bool dirty = true;  // the ring has been written since the last barrier: its initialisation, or a reload below
  for (u32 gi = 0; gi < count; gi++) {
    const K6R gnn = gi + 2 < count ? k6_range(P, first + gi + 2) : gn;
    uint4 p0{}, p1{}, p2{}, q0{}, q1{}, q2{};
    if (gi + 1 < count) {
      fetch(gn, 0, p0, q0);
      fetch(gn, 1, p1, q1);
      if (tid == 0) fetch(gn, 2, p2, q2);
    }
    if (g.hi > g.lo) {
      // 1. the window [need_lo, base): whatever of it the ring does not hold comes from memory, where it is final
      //    (octets of groups that needed no history, or octets this loop stored in an earlier step)
      if (!SYM) {
        const u64 need_lo = g.base - g.floor > K6_W ? g.base - K6_W : g.floor;
        if (!(w_hi == g.base && w_lo <= need_lo)) {
          dirty = true;
          const bool older = w_hi == g.base && w_lo < g.base;  // contiguous but short: the older part only
          const u64 upto = older ? w_lo : g.base;
          tbz_device_fence();  // (octets this workgroup stored in earlier steps must come back from L2, not a stale L1 line)
          tbz_wg_barrier();
          for (u64 x = need_lo + tid; x < upto; x += K6_THREADS) W0[(u32)((ob + x) & (K6_W - 1))] = P.out_base[x];
          w_lo = need_lo;
          if (!older) w_hi = g.base;
        }
      }
      if (dirty) tbz_wg_barrier();  // (workgroup-uniform; the step before ended in a barrier)
      dirty = false;
      // 2. gather first (a destination's ring slot is the slot of the source 32 KiB before it), then store.  Threads own
      //    16-octet chunks that are aligned in address space.
      const u32 rbase = (u32)(ob + g.base);
      auto src = [&](u32 idx, u32& a, u32& b) {
        const u32 r = (rbase + idx) & (K6_W - 1);
        a = W0[r];
        b = SYM ? (u32)W1[r] : 0u;
      };
      auto step_fix = [&](u32 k, uint4& o, uint4& m) -> bool {
        const u64 x = chunk_x(g, k);
        if ((i64)x >= (i64)g.hi) return false;
        if ((i64)x >= (i64)g.lo && x + 16 <= g.hi) return k6_fix16<true>(o, m, x, g.lo, g.hi, src);
        return k6_fix16<false>(o, m, x, g.lo, g.hi, src);
      };
      const bool c0 = step_fix(0, o0, m0), c1 = step_fix(1, o1, m1);
      bool c2 = false;
      if (tid == 0) c2 = step_fix(2, o2, m2);
      tbz_wg_barrier();
      auto step_store = [&](u32 k, const uint4& o, const uint4& m, bool chg) {
        const u64 x = chunk_x(g, k);
        if ((i64)x >= (i64)g.hi) return;
        if ((i64)x >= (i64)g.lo && x + 16 <= g.hi) {
          const u32 r = (u32)((ob + x) & (K6_W - 1));
          *(uint4*)(W0 + r) = o;
          if (SYM) *(uint4*)(W1 + r) = m;
          if (chg) {  // (final mode: the marks are now 0, so that tbz_k6_resolve leaves these octets alone)
            *(uint4*)(P.out_base + x) = o;
            *(uint4*)(P.mark_base + (x - P.bias)) = m;
          }
        } else {
          // the two ragged chunks at the ends: octet by octet — what lies outside [lo, hi) belongs to a neighbour
          // whose octets this copy (fetched a step early) may hold in an older state
          const u32 ow[4] = {o.x, o.y, o.z, o.w}, mw[4] = {m.x, m.y, m.z, m.w};
          for (u32 q = 0; q < 16; q++) {
            const u64 pos = x + q;
            if ((i64)pos < (i64)g.lo || (i64)pos >= (i64)g.hi) continue;
            const u8 b0 = (u8)(ow[q >> 2] >> (8 * (q & 3))), b1 = (u8)(mw[q >> 2] >> (8 * (q & 3)));
            const u32 r = (u32)((ob + pos) & (K6_W - 1));
            W0[r] = b0;
            if (SYM) W1[r] = b1;
            if (chg) {
              P.out_base[pos] = b0;
              P.mark_base[pos - P.bias] = b1;
            }
          }
        }
      };
      step_store(0, o0, m0, c0);
      step_store(1, o1, m1, c1);
      if (tid == 0) step_store(2, o2, m2, c2);
      if (w_hi < g.lo) w_lo = g.lo;                      // (final mode only: a gap — the ring restarts at this range)
      w_hi = g.hi;
      if (w_hi - w_lo > K6_W) w_lo = w_hi - K6_W;
      tbz_wg_barrier();
    }
    g = gn;
    gn = gnn;
    o0 = p0; o1 = p1; o2 = p2;
    m0 = q0; m1 = q1; m2 = q2;
  }
}

TBZ_KERNEL_WG(1024, 1) void tbz_k6_chain(K6Params P) {
  TBZ_SHARED __attribute__((aligned(16))) u8 W0[K6_W];
  k6_chain<false>(P, W0, W0);
}
TBZ_KERNEL_WG(1024, 1) void tbz_k6_chain_sym(K6Params P) {
  TBZ_SHARED __attribute__((aligned(16))) u8 W0[K6_W];
  TBZ_SHARED __attribute__((aligned(16))) u8 W1[K6_W];
  k6_chain<true>(P, W0, W1);
}

// ranges whose sources are final in memory, all in parallel (K6_PIECE octets per workgroup)
TBZ_KERNEL void tbz_k6_resolve(K6Params P) {
  const u32 lane = tbz_lane();
  const u32 ri = tbz_block() / P.pieces, piece = tbz_block() % P.pieces;
  if (ri >= P.n_ranges) return;
  const K6Range g = P.ranges[ri];
  if (g.hi <= g.lo) return;
  const uintptr_t ob = (uintptr_t)P.out_base;
  const u64 c_lo = g.lo - ((ob + g.lo) & 15);
  const u64 p_lo = c_lo + (u64)piece * K6_PIECE;
  if ((i64)p_lo >= (i64)g.hi) return;
  for (u32 k = lane; k < K6_PIECE / 16; k += 64) {
    const u64 x = p_lo + (u64)k * 16;
    if ((i64)x >= (i64)g.hi) break;
    uint4 m = *(const uint4*)(P.mark_base + (x - P.bias));
    if ((m.x | m.y | m.z | m.w) == 0) continue;
    uint4 o = *(const uint4*)(P.out_base + x);
    auto src = [&](u32 idx, u32& a, u32& b) {
      // (all sixteen lookups are made, symbolic or not: an address below the stream's first octet is one that no
      // pointer of a valid stream means — read the first octet instead of unmapped memory)
      const i64 y = (i64)(g.base - K6_W + idx);
      a = P.out_base[y < (i64)g.floor ? g.floor : (u64)y];
      b = 0;
    };
    const bool whole = (i64)x >= (i64)g.lo && x + 16 <= g.hi;
    if (!(whole ? k6_fix16<true>(o, m, x, g.lo, g.hi, src) : k6_fix16<false>(o, m, x, g.lo, g.hi, src))) continue;
    if ((i64)x >= (i64)g.lo && x + 16 <= g.hi) {
      *(uint4*)(P.out_base + x) = o;
    } else {  // ragged ends: the octets outside the range are another workgroup's
      const u32 ow[4] = {o.x, o.y, o.z, o.w};
      for (u32 q = 0; q < 16; q++)
        if ((i64)(x + q) >= (i64)g.lo && (i64)(x + q) < (i64)g.hi) P.out_base[x + q] = (u8)(ow[q >> 2] >> (8 * (q & 3)));
    }
  }
}

// The same for LONG ranges (the host picks by their mean length): four wavefronts per workgroup, the 32 KiB that the
// range's pointers refer to staged in LDS once — tbz_k6_resolve's lookups are sixteen scattered one-octet loads from
// memory per chunk — then K6R_PIECE octets of the range are walked.  (Short ranges: staging 32 KiB costs more than it saves.)
constexpr u32 K6R_THREADS = 256;
constexpr u32 K6R_PIECE = 65536;
TBZ_KERNEL_WG(256, 2) void tbz_k6_resolve_lds(K6Params P) {
  TBZ_SHARED __attribute__((aligned(16))) u8 win[K6_W];
  const u32 tid = tbz_wave() * 64 + tbz_lane();
  const u32 ri = tbz_block() / P.pieces, piece = tbz_block() % P.pieces;
  if (ri >= P.n_ranges) return;  // (workgroup-uniform, like the two below: no barrier is left waiting)
  const K6Range g = P.ranges[ri];
  if (g.hi <= g.lo) return;
  const uintptr_t ob = (uintptr_t)P.out_base;
  const u64 c_lo = g.lo - ((ob + g.lo) & 15);
  const u64 p_lo = c_lo + (u64)piece * K6R_PIECE;
  if ((i64)p_lo >= (i64)g.hi) return;
  // pointer i stands for the octet at base - 32768 + i; an address below the stream's first octet is one that no
  // pointer of a valid stream means: the first octet stands in for it
  const i64 w0 = (i64)g.base - (i64)K6_W;
  for (u32 i = tid * 16; i < K6_W; i += K6R_THREADS * 16) {
    const i64 y = w0 + (i64)i;
    if (y >= (i64)g.floor) {
      *(K2U128*)(win + i) = *(const K2U128*)(P.out_base + y);
    } else {
      for (u32 q = 0; q < 16; q++) win[i + q] = P.out_base[y + q < (i64)g.floor ? g.floor : (u64)(y + q)];
    }
  }
  tbz_wg_barrier();
  for (u32 k = tid; k < K6R_PIECE / 16; k += K6R_THREADS) {
    const u64 x = p_lo + (u64)k * 16;
    if ((i64)x >= (i64)g.hi) break;
    uint4 m = *(const uint4*)(P.mark_base + (x - P.bias));
    if ((m.x | m.y | m.z | m.w) == 0) continue;
    uint4 o = *(const uint4*)(P.out_base + x);
    auto src = [&](u32 idx, u32& a, u32& b) {  // (all sixteen lookups are made, symbolic or not)
      a = win[idx & (K6_W - 1)];
      b = 0;
    };
    const bool whole = (i64)x >= (i64)g.lo && x + 16 <= g.hi;
    if (!(whole ? k6_fix16<true>(o, m, x, g.lo, g.hi, src) : k6_fix16<false>(o, m, x, g.lo, g.hi, src))) continue;
    if (whole) {
      *(uint4*)(P.out_base + x) = o;
    } else {  // ragged ends: the octets outside the range are another workgroup's
      const u32 ow[4] = {o.x, o.y, o.z, o.w};
      for (u32 q = 0; q < 16; q++)
        if ((i64)(x + q) >= (i64)g.lo && (i64)(x + q) < (i64)g.hi) P.out_base[x + q] = (u8)(ow[q >> 2] >> (8 * (q & 3)));
    }
  }
}

// ================================================================================================
// K3 — layout on the device for the common case.  After K1 the host must chain the items of each
// stream (did item k land exactly on item k+1?), lay the segments out in the output and describe
// the work to K2.  When every item of every stream simply LANDED on its successor, the last one
// decoded the final block and no match reaches behind its own segment, that chain is the identity:
// these kernels prove it, scan the segment sizes and write K2's Seg/Group tables themselves, so
// the host reads back one small record per stream instead of walking 64 bytes per segment.
// Anything else (false markers, repairs, sync-flush history, errors) -> glob.not_simple
// and the host's general path decides.
// ================================================================================================
constexpr u32 K3_TILE = 1024;  // items per workgroup
struct K3Stream {              // per stream, written by the device
  u64 total_out, tok_words, nonempty;
  SegResult last;              // result of the stream's last item (trailer, end position)
  u64 last_start;              // where that item starts (bit): the last flush boundary the chain landed on
};
struct K3Global {               // per launch of tbz_k3_scan_tiles: over the tiles of that launch only, but for total_out
  u32 not_simple, n_big;
  u64 max_small;               // largest group that fits the linear K2 window
  u64 max_out, total_out;      // largest item / all items up to the launch's last tile (octets): the host slices segments
                               // that are far too large
};
struct K3Params {
  const Item* items;
  const SegResult* res;
  const u32* first_item;       // per stream
  const u32* n_items_s;
  const u64* out_off;
  const u64* out_cap;
  u64* tile_sums;              // [3][n_tiles + 1]: out_bytes, tok_words, nonempty; scanned in place
  u64* tile_flags;             // [4][n_tiles]: not_simple, n_big, max_small, max_out
  u64* gscan;                  // [n_items]: exclusive scan of out_bytes over ALL items
  u32* gne;                    // [n_items]: exclusive scan of the non-empty flags
  Seg* segs;
  Group* groups;
  K3Stream* streams;
  K3Global* glob;
  u32 n_items, n_tiles, n_streams;
  // ---- the tiles [t0, t1) this launch covers (the whole call: 0, n_tiles).  The call's tiles may be laid out in several
  // launches in ascending order: the tile scan continues from the totals the launch before it left in `carry`
  u32 t0, t1;
  u64* carry;                  // [3]: out_bytes, tok_words, nonempty of the tiles before t1
};

TBZ_KERNEL void tbz_k3_tile_sums(K3Params P) {
  const u32 lane = tbz_lane(), t = P.t0 + tbz_block();
  u64 so = 0, sw = 0, sn = 0, bad = 0, nbig = 0, mx = 0, mxo = 0;
  for (u32 it = 0; it < K3_TILE / 64; it++) {
    const u32 i = t * K3_TILE + it * 64 + lane;
    if (i >= P.n_items) continue;
    const SegResult q = P.res[i];
    const u32 s = P.items[i].stream;
    const bool last = i - P.first_item[s] == P.n_items_s[s] - 1;
    // (a last item that ran out of input is as good as one that met the final block: its tokens stand)
    const bool ok = (q.status == (last ? SEG_FINAL : SEG_LANDED) || (last && q.status == SEG_UNDERRUN)) && q.max_deficit == 0;
    bad |= ok ? 0u : 1u;
    so += q.out_bytes;
    sw += q.tok_words;
    sn += (q.out_bytes | q.tok_words) ? 1u : 0u;
    const bool big = q.out_bytes + K2_SLACK > K2_SMALL_MAX;
    nbig += big ? 1u : 0u;
    mx = !big && q.out_bytes > mx ? q.out_bytes : mx;
    mxo = q.out_bytes > mxo ? q.out_bytes : mxo;
  }
  so = wave_sum_u64(so);
  sw = wave_sum_u64(sw);
  sn = wave_sum_u64(sn);
  bad = wave_sum_u64(bad);
  nbig = wave_sum_u64(nbig);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const u64 o = tbz_shfl_xor64(mx, m);
    mx = o > mx ? o : mx;
    const u64 o2 = tbz_shfl_xor64(mxo, m);
    mxo = o2 > mxo ? o2 : mxo;
  }
  if (lane == 0) {
    const u32 T1 = P.n_tiles + 1;
    P.tile_sums[t] = so;
    P.tile_sums[T1 + t] = sw;
    P.tile_sums[2 * T1 + t] = sn;
    P.tile_flags[t] = bad;
    P.tile_flags[P.n_tiles + t] = nbig;
    P.tile_flags[2 * P.n_tiles + t] = mx;
    P.tile_flags[3 * P.n_tiles + t] = mxo;
  }
}

// single wave: exclusive scan of the tile sums, reduction of the flags
TBZ_KERNEL void tbz_k3_scan_tiles(K3Params P) {
  const u32 lane = tbz_lane();
  const u32 T1 = P.n_tiles + 1;
  u64 total_out = 0;
  for (u32 c = 0; c < 3; c++) {
    u64 carry = P.t0 ? P.carry[c] : 0;
    for (u32 i = P.t0; i < P.t1; i += 64) {
      const u64 v = (i + lane) < P.t1 ? P.tile_sums[c * T1 + i + lane] : 0;
      const u64 inc = wave_incl_scan_u64(v);
      if ((i + lane) < P.t1) P.tile_sums[c * T1 + i + lane] = carry + inc - v;
      carry += tbz_shfl64(inc, 63);
    }
    if (lane == 0) {
      P.carry[c] = carry;
      if (P.t1 == P.n_tiles) P.tile_sums[c * T1 + P.n_tiles] = carry;
    }
    if (c == 0) total_out = carry;
  }
  u64 bad = 0, nbig = 0, mx = 0, mxo = 0;
  for (u32 i = P.t0 + lane; i < P.t1; i += 64) {
    bad += P.tile_flags[i];
    nbig += P.tile_flags[P.n_tiles + i];
    const u64 m = P.tile_flags[2 * P.n_tiles + i];
    mx = m > mx ? m : mx;
    const u64 m2 = P.tile_flags[3 * P.n_tiles + i];
    mxo = m2 > mxo ? m2 : mxo;
  }
  bad = wave_sum_u64(bad);
  nbig = wave_sum_u64(nbig);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const u64 o = tbz_shfl_xor64(mx, m);
    mx = o > mx ? o : mx;
    const u64 o2 = tbz_shfl_xor64(mxo, m);
    mxo = o2 > mxo ? o2 : mxo;
  }
  if (lane == 0) {
    K3Global gl;
    gl.not_simple = bad ? 1u : 0u;
    gl.n_big = (u32)nbig;
    gl.max_small = mx;
    gl.max_out = mxo;
    gl.total_out = total_out;
    *P.glob = gl;
  }
}

// exclusive scans of out_bytes and of the non-empty flags over all items (tile prefix + in-tile scan in item order)
TBZ_KERNEL void tbz_k3_scan_items(K3Params P) {
  const u32 lane = tbz_lane(), t = P.t0 + tbz_block();
  u64 carry = P.tile_sums[t];
  u32 carry_ne = (u32)P.tile_sums[2 * (P.n_tiles + 1) + t];
  for (u32 it = 0; it < K3_TILE / 64; it++) {
    const u32 i = t * K3_TILE + it * 64 + lane;
    u64 v = 0;
    u32 ne = 0;
    if (i < P.n_items) {
      const SegResult q = P.res[i];
      v = q.out_bytes;
      ne = (q.out_bytes | q.tok_words) ? 1u : 0u;
    }
    const u64 inc = wave_incl_scan_u64(v);
    const u32 inc_ne = wave_incl_scan_u32(ne);
    if (i < P.n_items) {
      P.gscan[i] = carry + inc - v;
      P.gne[i] = carry_ne + inc_ne - ne;
    }
    carry += tbz_shfl64(inc, 63);
    carry_ne += tbz_shfl(inc_ne, 63);
  }
}

// one Seg and one Group per item; the lane of a stream's last item writes the stream's record (the stream's first item
// may lie in a tile of an earlier launch: its gscan / gne entries are there by then)
TBZ_KERNEL void tbz_k3_emit(K3Params P) {
  const u32 lane = tbz_lane(), t = P.t0 + tbz_block();
  const u32 T1 = P.n_tiles + 1;
  for (u32 it = 0; it < K3_TILE / 64; it++) {
    const u32 i = t * K3_TILE + it * 64 + lane;
    if (i >= P.n_items) continue;
    const SegResult q = P.res[i];
    const Item im = P.items[i];
    const u32 s = im.stream, f = P.first_item[s];
    const u64 rel = P.gscan[i] - P.gscan[f];
    Seg sg;
    sg.tok = q.tok;
    sg.tok_words = q.tok_words;
    sg.out_bytes = q.out_bytes;
    sg.n_runs = q.n_runs;
    sg.run_first = 0;
    sg.runs = q.runs;
    sg.run0 = q.run0;
    P.segs[i] = sg;
    Group g;
    g.out_abs = P.out_off[s] + rel;
    g.out_end = P.out_off[s] + P.out_cap[s];
    g.seg_first = i;
    g.seg_count = 1;
    P.groups[i] = g;
    if (i - f == P.n_items_s[s] - 1) {
      K3Stream st;
      st.total_out = rel + q.out_bytes;
      st.tok_words = 0;   // token words are only totalled for the whole call (below)
      st.nonempty = P.gne[i] - P.gne[f] + ((q.out_bytes | q.tok_words) ? 1u : 0u);
      st.last = q;
      st.last_start = im.start_bit;
      P.streams[s] = st;
    }
  }
  if (t == P.n_tiles - 1 && lane == 0) {  // whole-call totals ride in the slot after the last stream (the last launch's)
    K3Stream tot;
    tot.total_out = P.tile_sums[P.n_tiles];
    tot.tok_words = P.tile_sums[T1 + P.n_tiles];
    tot.nonempty = P.tile_sums[2 * T1 + P.n_tiles];
    tot.last = SegResult{};
    tot.last_start = 0;
    P.streams[P.n_streams] = tot;
  }
}

// ================================================================================================
// K3s — slices.  K2's parallelism is its number of groups, and a segment is as large as the encoder's blocks (or the
// whole stream, when nothing in it can be found: fixed-Huffman or stored blocks without flush points).  A large
// segment is therefore cut at RUN boundaries (K1 left the octets each run produces and how far its matches reach
// back in the run table) into units of about `target` octets: run i, which starts P_i octets into the segment,
// belongs to slice floor(P_i / target).  Each slice becomes a group of its own; one that reaches before its first
// octet is an H-group (symbolic history + K6), exactly like a segment that reaches into the segment before it.
// One wavefront per segment; the host reads the small per-slice records back and schedules K2 / K6 from them.
// ================================================================================================
struct BigSeg {
  Seg seg;          // the whole segment
  u64 out_abs;      // absolute output offset of its first octet
  u64 out_end;      // clip (the stream's capacity)
  u64 target;       // octets per slice
  u32 seg_slot;     // slices go to segs[seg_slot + k], groups[group_slot + k], recs[rec_slot + k], k < n_slots
  u32 group_slot;
  u32 rec_slot;
  u32 n_slots;
  u32 first_hist;   // 1: the segment itself reaches before its first octet (slice 0 is an H-group)
  u32 pad;
};
struct SliceRec {
  u64 out_abs;
  u64 out_bytes;
  u32 hist;
  u32 used;
};
struct K3sParams {
  const BigSeg* big;
  Seg* segs;
  Group* groups;
  SliceRec* recs;
  u32 n_big;
};
TBZ_KERNEL void tbz_k3_slice(K3sParams P) {
  const u32 lane = tbz_lane();
  if (tbz_block() >= P.n_big) return;
  const BigSeg bs = P.big[tbz_block()];
  const RunRec* rt = (const RunRec*)bs.seg.runs;
  for (u32 k = lane; k < bs.n_slots; k += 64) {  // slots no run starts in stay empty
    Group g{};
    g.out_abs = bs.out_abs;
    g.out_end = bs.out_abs;
    g.seg_first = bs.seg_slot + k;
    g.seg_count = 0;
    P.groups[bs.group_slot + k] = g;
    P.recs[bs.rec_slot + k] = SliceRec{};
  }
  tbz_sync();
  // the slice being accumulated (wave-uniform)
  u64 cur_k = ~0ull, cur_start = 0, acc_words = 0, acc_out = 0, carry = 0;
  u32 cur_first = 0, cur_runs = 0, cur_hist = 0;
  auto flush = [&]() {
    if (cur_k == ~0ull || cur_runs == 0 || cur_k >= bs.n_slots) return;
    if (lane == 0) {
      Seg sg = bs.seg;
      sg.tok_words = acc_words;
      sg.out_bytes = acc_out;
      sg.n_runs = cur_runs;
      sg.run_first = cur_first;
      P.segs[bs.seg_slot + cur_k] = sg;
      Group g;
      g.out_abs = bs.out_abs + cur_start;
      g.out_end = bs.out_end;
      g.seg_first = bs.seg_slot + (u32)cur_k;
      g.seg_count = 1;
      P.groups[bs.group_slot + cur_k] = g;
      SliceRec r;
      r.out_abs = bs.out_abs + cur_start;
      r.out_bytes = acc_out;
      r.hist = cur_k == 0 ? bs.first_hist : cur_hist;
      r.used = 1;
      P.recs[bs.rec_slot + cur_k] = r;
    }
  };
  for (u32 base = 0; base < bs.seg.n_runs; base += 64) {  // wave-uniform trip count
    RunRec rr{};
    const bool have = base + lane < bs.seg.n_runs;
    if (have) rr = (base + lane) ? rt[base + lane] : bs.seg.run0;
    const u64 incl_o = wave_incl_scan_u64(rr.out), incl_w = wave_incl_scan_u64((u64)rr.n8 * 8);
    const u64 Pi = carry + incl_o - rr.out;  // octets of the segment before this run
    const u64 ki = Pi / bs.target;
    const u32 kprev_lo = tbz_wave_shr1((u32)ki), kprev_hi = tbz_wave_shr1((u32)(ki >> 32));
    const u64 kprev = lane == 0 ? cur_k : (((u64)kprev_hi << 32) | kprev_lo);
    u64 heads = tbz_ballot(have && ki != kprev);
    const u64 valid = tbz_ballot(have);
    u32 from = 0;
    // the chunk's runs go to the current slice up to the first head, then slice by slice
    for (;;) {
      const u32 to = heads ? (u32)tbz_ffs64(heads) - 1 : (u32)tbz_popc64(valid);  // lanes [from, to) continue the slice
      if (to > from) {
        const u64 o_hi = tbz_shfl64(incl_o, (int)(to - 1)), w_hi = tbz_shfl64(incl_w, (int)(to - 1));
        const u64 o_lo = from ? tbz_shfl64(incl_o, (int)(from - 1)) : 0, w_lo = from ? tbz_shfl64(incl_w, (int)(from - 1)) : 0;
        const bool in = lane >= from && lane < to;
        // a run reaches before the slice's first octet when its matches reach further back than it is into the slice
        const u64 reach = tbz_ballot(in && (u64)rr.mdef > Pi - cur_start);
        acc_out += o_hi - o_lo;
        acc_words += w_hi - w_lo;
        cur_runs += to - from;
        cur_hist |= reach ? 1u : 0u;
      }
      if (!heads) break;
      flush();
      const u32 h = (u32)tbz_ffs64(heads) - 1;
      heads &= heads - 1;
      cur_k = tbz_shfl64(ki, (int)h);
      cur_start = tbz_shfl64(Pi, (int)h);
      cur_first = base + h;
      cur_runs = 0;
      cur_hist = 0;
      acc_words = acc_out = 0;
      from = h;
    }
    carry += tbz_shfl64(incl_o, 63);
  }
  flush();
}

// ================================================================================================
// K4 — adler32 (checksums.lisp:18-62).  Partials per 64 KiB chunk, then an ordered combine.
//   A = sum b_i, B = sum (n - i) * b_i  (i = 0..n-1), both mod 65521
// ================================================================================================
struct K4Params {
  const u8* out_base;
  const CkChunk* chunks;
  CkPartial* parts;
  u32 n_chunks;
};

// (A, B) = (sum of the octets, sum of (n - i) * octet) of p[0, n), each mod 65521, on every lane: one chunk's share of
// an adler32 (checksums.lisp:18-62 split so that chunks combine)
TBZ_DEV void k4_adler_chunk(const u8* p, u32 n, u32& a_out, u32& b_out) {
  const u32 lane = tbz_lane();
  u32 head = (u32)((0 - (uintptr_t)p) & 15);
  if (head > n) head = n;
  u32 body = (n - head) & ~15u;
  u64 A = 0, B = 0;
  if (lane < head) {
    u32 b = p[lane];
    A += b;
    B += (u64)(n - lane) * b;
  }
  const uint4* q = (const uint4*)(p + head);
  for (u32 c = lane; c < (body >> 4); c += 64) {
    uint4 v = q[c];
    u32 i0 = head + c * 16;
    u32 wv[4] = {v.x, v.y, v.z, v.w};
    u32 a16 = 0, w16 = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
      u32 b = (wv[k >> 2] >> ((k & 3) * 8)) & 0xff;
      a16 += b;
      w16 += k * b;
    }
    A += a16;
    B += (u64)(n - i0) * a16 - w16;
  }
  u32 t0 = head + body;
  if (t0 + lane < n) {
    u32 b = p[t0 + lane];
    A += b;
    B += (u64)(n - t0 - lane) * b;
  }
  A = wave_sum_u64(A);
  B = wave_sum_u64(B % ADLER_P);
  a_out = (u32)(A % ADLER_P);
  b_out = (u32)(B % ADLER_P);
}
TBZ_KERNEL void tbz_k4_adler_partial(K4Params P) {
  if (tbz_block() >= P.n_chunks) return;
  const CkChunk ch = P.chunks[tbz_block()];
  CkPartial r;
  k4_adler_chunk(P.out_base + ch.out_abs, ch.len, r.a, r.b);
  if (tbz_lane() == 0) P.parts[tbz_block()] = r;
}

struct K4cParams {
  const CkChunk* chunks;
  const CkPartial* parts;
  const CkStream* streams;
  u32* out;  // per stream: s1 | s2 << 16
  u32 n_streams;
};
TBZ_KERNEL void tbz_k4_adler_combine(K4cParams P) {
  if (tbz_block() >= P.n_streams) return;
  const u32 lane = tbz_lane();
  const CkStream cs = P.streams[tbz_block()];
  // everything fits 32 bits: partials and n mod P are < 65521, a row's prefix sum < 64 * 65521, and
  // (P-1)^2 + (P-1) < 2^32
  u32 s1 = cs.init0 & 0xffff, s2 = cs.init0 >> 16;  // running, < P
  for (u32 c0 = 0; c0 < cs.count; c0 += 256) {  // four rows of 64 chunks per trip: their loads go out together
    u32 a[4], b[4], n[4];
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
      const u32 c = c0 + q * 64 + lane;
      const bool v = c < cs.count;
      a[q] = v ? P.parts[cs.first + c].a : 0;
      b[q] = v ? P.parts[cs.first + c].b : 0;
      n[q] = v ? P.chunks[cs.first + c].len % ADLER_P : 0;
    }
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
      const u32 inc = tbz_wave_incl_scan_u32(a[q]);
      const u32 s1_before = (s1 + inc - a[q]) % ADLER_P;
      const u32 term = (n[q] * s1_before + b[q]) % ADLER_P;  // absent chunks: n = b = 0
      const u32 tsum = tbz_shfl(tbz_wave_incl_scan_u32(term), 63);
      s2 = (s2 + tsum) % ADLER_P;
      s1 = (s1 + tbz_shfl(inc, 63)) % ADLER_P;
    }
  }
  if (lane == 0) P.out[tbz_block()] = (u32)s1 | ((u32)s2 << 16);
}

// the same combine over a RANGE of chunks, leaving a partial again ({A, B} and the range's length): level 1 of the
// two-level combine used when K2 hands over one partial per group (65 536 of them for 1 GiB)
struct K4lParams {
  const CkChunk* chunks;
  const CkPartial* parts;
  const CkStream* ranges;  // first / count; init0 unused
  CkChunk* out_chunks;
  CkPartial* out_parts;
  u32 n_ranges;
};
TBZ_KERNEL void tbz_k4_adler_combine_l1(K4lParams P) {
  if (tbz_block() >= P.n_ranges) return;
  const u32 lane = tbz_lane();
  const CkStream cs = P.ranges[tbz_block()];
  u32 s1 = 0, s2 = 0;
  u64 total = 0;
  for (u32 c0 = 0; c0 < cs.count; c0 += 256) {
    u32 a[4], b[4], n[4];
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
      const u32 c = c0 + q * 64 + lane;
      const bool v = c < cs.count;
      a[q] = v ? P.parts[cs.first + c].a : 0;
      b[q] = v ? P.parts[cs.first + c].b : 0;
      n[q] = v ? P.chunks[cs.first + c].len : 0;
    }
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
      total += wave_sum_u64(n[q]);
      const u32 inc = tbz_wave_incl_scan_u32(a[q]);
      const u32 s1_before = (s1 + inc - a[q]) % ADLER_P;
      const u32 term = ((n[q] % ADLER_P) * s1_before + b[q]) % ADLER_P;
      const u32 tsum = tbz_shfl(tbz_wave_incl_scan_u32(term), 63);
      s2 = (s2 + tsum) % ADLER_P;
      s1 = (s1 + tbz_shfl(inc, 63)) % ADLER_P;
    }
  }
  if (lane == 0) {
    CkPartial r;
    r.a = s1;
    r.b = s2;
    P.out_parts[tbz_block()] = r;
    CkChunk ch;
    ch.out_abs = 0;
    ch.len = (u32)total;
    ch.stream = 0;
    P.out_chunks[tbz_block()] = ch;
  }
}

// ================================================================================================
// K5 — crc32 (checksums.lisp:177-210), reflected polynomial 0xedb88320.
// Z = "advance the register by one zero octet" = multiplication by x^8 mod P.  With init 0,
//   r(M) = XOR_i Z^(n-1-i) T[b_i]     and    r(A||B) = Z^|B| r(A) ^ r(B).
// A chunk is read as 256-byte rows, lane j taking word j of each row (fully coalesced); each lane
// runs S <- Z^256(S) ^ word (4 LDS lookups), then lanes are aligned with one constant multiply each.
// ================================================================================================
TBZ_DEV u32 crc_mulmod(u32 a, u32 b) {  // a*b mod P, reflected (bit 31 = x^0)
  u32 p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1) ? ((b >> 1) ^ 0xedb88320u) : (b >> 1);
  }
  return p;
}
TBZ_DEV u32 crc_pow_x8(const u32* x2n, u64 nbytes) {  // x^(8*nbytes) mod P
  u32 p = 0x80000000u;
  u32 k = 3;
  while (nbytes) {
    if (nbytes & 1) p = crc_mulmod(x2n[k & 63], p);
    nbytes >>= 1;
    k++;
  }
  return p;
}
TBZ_DEV u32 crc_bytes_seq(const u32* T, const u8* p, u32 n) {  // r() of n octets, one lookup per octet
  u32 s = 0;
  for (u32 i = 0; i < n; i++) s = (s >> 8) ^ T[(s ^ p[i]) & 0xff];
  return s;
}

struct K5Params {
  const u8* out_base;
  const CkChunk* chunks;
  CkPartial* parts;
  const u32* crc_tab;  // CRC_WORDS words (tbz_structs.hpp)
  u32 n_chunks;
};

// raw CRC-32 (initial value 0, no final complement) of p[0, n) on every lane; tab = the first CRC_X2N words of the
// constant table in LDS, crc_tab the whole of it in memory
TBZ_DEV u32 k5_crc_chunk(const u32* tab, const u32* crc_tab, const u8* p, u32 n) {
  const u32 lane = tbz_lane();
  u32 head = (u32)((0 - (uintptr_t)p) & 3);
  if (head > n) head = n;
  u32 rows = (n - head) >> 8;
  u32 tail = n - head - rows * 256;
  const u32* q = (const u32*)(p + head);
  const u32* K = tab + CRC_K;
  u32 S = 0;
  for (u32 r = 0; r < rows; r++) {
    u32 w = q[r * 64 + lane];
    S = K[S & 0xff] ^ K[256 + ((S >> 8) & 0xff)] ^ K[512 + ((S >> 16) & 0xff)] ^ K[768 + (S >> 24)] ^ w;
  }
  u32 rr = 0;
  if (rows) {
    rr = crc_mulmod(crc_tab[CRC_LANE + lane], S);
    rr = wave_xor_u32(rr);
  }
  // wave-uniform from here
  u32 rtot = rr;
  if (head) {
    u32 rh = crc_bytes_seq(tab, p, head);
    rtot ^= crc_mulmod(crc_pow_x8(crc_tab + CRC_X2N, (u64)rows * 256), rh);
  }
  if (tail) {
    u32 rt = crc_bytes_seq(tab, p + head + rows * 256, tail);
    rtot = crc_mulmod(crc_pow_x8(crc_tab + CRC_X2N, tail), rtot) ^ rt;
  }
  return rtot;
}
TBZ_KERNEL void tbz_k5_crc_partial(K5Params P) {
  TBZ_SHARED u32 tab[CRC_X2N];  // T + K0..K3
  const u32 lane = tbz_lane();
  for (u32 i = lane; i < CRC_X2N; i += 64) tab[i] = P.crc_tab[i];
  tbz_sync();
  if (tbz_block() >= P.n_chunks) return;
  const CkChunk ch = P.chunks[tbz_block()];
  const u32 rtot = k5_crc_chunk(tab, P.crc_tab, P.out_base + ch.out_abs, ch.len);
  if (lane == 0) {
    CkPartial o;
    o.a = rtot;
    o.b = 0;
    P.parts[tbz_block()] = o;
  }
}

struct K5cParams {
  const CkChunk* chunks;
  const CkPartial* parts;
  const CkStream* streams;
  const u32* crc_tab;
  u32* out;  // per stream: finalised crc
  u32 n_streams;
};
TBZ_KERNEL void tbz_k5_crc_combine(K5cParams P) {
  if (tbz_block() >= P.n_streams) return;
  const u32 lane = tbz_lane();
  const CkStream cs = P.streams[tbz_block()];
  const u32* x2n = P.crc_tab + CRC_X2N;
  // octets after chunk c = suffix sum of lengths; lanes take chunks round-robin
  u64 total = 0;
  for (u32 c0 = 0; c0 < cs.count; c0 += 64) {
    u32 c = c0 + lane;
    total += wave_sum_u64(c < cs.count ? P.chunks[cs.first + c].len : 0);
  }
  u32 acc = 0;
  u64 before = 0;
  for (u32 c0 = 0; c0 < cs.count; c0 += 64) {
    u32 c = c0 + lane;
    bool v = c < cs.count;
    u64 n = v ? P.chunks[cs.first + c].len : 0;
    u64 inc = wave_incl_scan_u64(n);
    u64 after = total - (before + inc);
    if (v) acc ^= crc_mulmod(crc_pow_x8(x2n, after), P.parts[cs.first + c].a);
    before += tbz_shfl64(inc, 63);
  }
  acc = wave_xor_u32(acc);
  // crc' = ~( Z^n(~crc) ^ r(M) )  — chaining convention of crc32/table (checksums.lisp:201,:210)
  u32 init = cs.init0 ^ 0xffffffffu;
  u32 fin = crc_mulmod(crc_pow_x8(x2n, total), init) ^ acc;
  if (lane == 0) P.out[tbz_block()] = fin ^ 0xffffffffu;
}

// ================================================================================================
// tbz_small_fused — ONE launch for one small stream (round 4; VERDICT r3 item 5: the call floor).
//
// The general pipeline is a dozen launches and three host read-backs whatever the size of the call: 0.2 ms for config 1's
// one stored block of 65 535 octets, below the one-core CPU rate.  A stream that is small AND has no flush points is one
// K1 item and one K2 group anyway, so one workgroup can do everything in turn: look for flush markers (any: not this
// kernel's case), decode the item with a gang of 64 (k1g_body: header, tables, rounds, commit), lay the one segment out,
// resolve LZ77 through the ring window (k2_body), take the checksum of the output and compare it with the trailer.  The
// host reads ONE record.  It decides nothing but the clean case — the final block decoded, the trailer complete and
// matching, everything fits, no match reaches before the stream's first octet — anything else says "fall back" and the
// general path runs, so every flag, count and error of the reference is still produced by the code the parity suites
// pin.  (deflate.lisp:92-730 / zlib.lisp:80-143 / gzip.lisp:110-286 front to back, for one stream.)
// ================================================================================================
constexpr u32 SMALL_MAX_OUT = 256u << 10;  // one wave resolves and checks the output: bounded (CK_CHUNK, one checksum chunk)
static_assert(SMALL_MAX_OUT <= CK_CHUNK, "one checksum chunk");
enum { SMALL_DONE = 1, SMALL_FALLBACK = 2 };
struct SmallRec {
  u32 state;   // SMALL_DONE: `seg` and `check` describe the finished stream; SMALL_FALLBACK: decode it the general way
  u32 check;   // adler32 (s1 | s2 << 16) / crc32 of the output (equal to the trailer's), 0 for raw deflate
  u32 why;     // diagnostics: which rule sent the stream to the general path
  u32 pad;
  SegResult seg;
};
struct SmallParams {
  const u8* in;
  u64 in_len;
  u8* out;
  u64 out_cap;
  u32 format;
  u32 find_min;   // streams of at least this many octets that do not begin with a stored block belong to the block-start finder
  u16* tok;       // token pool for this stream: (in_len * 8 >> 1) + 64 words (one word per two input bits)
  RunRec* runs;   // run table: (in_len * 8 >> RUN_SHIFT) + 2 entries
  const u32* crc_tab;
  SmallRec* rec;
};
struct SmallK2Lds {
  __attribute__((aligned(16))) u8 win[K2R_RW];
  __attribute__((aligned(16))) u8 idt[K2_IDT];
  __attribute__((aligned(16))) u16 tks[K2_TOKBUF];
  u32 rcache[128];
};
union SmallLds {  // (the stages run one after the other)
  KgLds<64> k1;
  SmallK2Lds k2;
  u32 crc[CRC_X2N];
};

// any 00 00 FF FF in p[0, n)?  (sixteen start positions per lane and trip: four v_qsad_pk_u16_u8 against the pattern)
TBZ_DEV bool small_has_marker(const u8* p, u64 n) {
  const u32 lane = tbz_lane();
  bool hit = false;
  // whole 16-octet chunks whose four octets of lookahead are inside the stream
  const u64 chunks = n >= 20 ? (n - 4) / 16 : 0;
  for (u64 c0 = 0; c0 < chunks; c0 += 64) {
    const u64 c = c0 + lane;
    if (c < chunks) {
      const u8* q = p + c * 16;
      const u64 lo = k2_ld64(q), hi = k2_ld64(q + 8);
      const u32 nx = k2_ld32(q + 16);
      const u64 w0 = lo, w1 = (lo >> 32) | (hi << 32), w2 = hi, w3 = (hi >> 32) | ((u64)nx << 32);
      const u64 s = tbz_qsad4(w0, 0xFFFF0000u), t = tbz_qsad4(w1, 0xFFFF0000u), u = tbz_qsad4(w2, 0xFFFF0000u), v = tbz_qsad4(w3, 0xFFFF0000u);
      // a zero 16-bit field is an exact match
      const u32 m = tbz_pk_min_u16(tbz_pk_min_u16((u32)s, (u32)(s >> 32)), tbz_pk_min_u16((u32)t, (u32)(t >> 32)));
      const u32 m2 = tbz_pk_min_u16(tbz_pk_min_u16((u32)u, (u32)(u >> 32)), tbz_pk_min_u16((u32)v, (u32)(v >> 32)));
      const u32 mm = tbz_pk_min_u16(m, m2);
      hit = hit | ((mm & 0xffffu) == 0) | ((mm >> 16) == 0);
    }
  }
  // the last octets, one start position per lane
  const u64 t0 = chunks * 16;
  for (u64 i = t0 + lane; i + 4 <= n; i += 64) hit = hit | (p[i] == 0 && p[i + 1] == 0 && p[i + 2] == 0xff && p[i + 3] == 0xff);
  return tbz_ballot(hit) != 0;
}

TBZ_KERNEL_OCC(2) void tbz_small_fused(SmallParams P) {
  TBZ_SHARED SmallLds S;
  TBZ_SHARED Item s_item;
  TBZ_SHARED SegResult s_res;
  TBZ_SHARED u32 s_fm[2];
  const u32 lane = tbz_lane();
  auto leave = [&](u32 state, u32 check, u32 why) {
    if (lane == 0) {
      SmallRec r;
      r.state = state;
      r.check = check;
      r.why = why;
      r.pad = 0;
      r.seg = s_res;
      *P.rec = r;
    }
  };
  if (lane == 0) {
    s_res = SegResult{};
    s_fm[0] = s_fm[1] = 0;
    Item it{};
    it.start_bit = 0;
    it.limit_bit = ~0ull;
    it.end_byte = P.in_len;
    it.stream = 0;
    it.flags = (P.format << ITEM_FMT_SHIFT) | ITEM_HEAD;
    s_item = it;
  }
  tbz_sync();
  // ---- a stream that is nothing but stored blocks (deflate.lisp:532-573; incompressible data: config 1) needs neither
  // tokens nor a window: this wave walks the headers and copies input to output as it goes.  Anything that is not a
  // plain chain to a final block inside the buffers leaves the decision to the code below (which decodes from the
  // start again: whatever this copied is overwritten).
  bool chain = false;
  if (P.format != 2) {
    u64 at = 0;
    bool ok = true;
    if (P.format == 1) {  // the zlib header exactly as K1 accepts it (zlib.lisp:20-35), or not this path's stream
      ok = P.in_len >= 2 && (P.in[0] & 15) == 8 && (P.in[0] >> 4) <= 7 && (P.in[1] & 0x20) == 0 &&
           (((u32)P.in[0] << 8) | P.in[1]) % 31 == 0;
      at = 2;
    }
    u64 o = 0;
    bool fin = false;
    while (ok && !fin) {
      if (at + 5 > P.in_len) { ok = false; break; }
      const u32 h = P.in[at];
      const u32 len = P.in[at + 1] | ((u32)P.in[at + 2] << 8), nlen = P.in[at + 3] | ((u32)P.in[at + 4] << 8);
      if (((h >> 1) & 3) != 0 || (len ^ nlen) != 0xffffu) { ok = false; break; }
      if (len == 0 && !(h & 1)) { ok = false; break; }  // an empty stored block is a flush point: the general path counts it
      if (at + 5 + len > P.in_len || o + len > P.out_cap || o + len > SMALL_MAX_OUT) { ok = false; break; }
      fin = (h & 1) != 0;
      const u8* in = P.in + at + 5;
      u8* out = P.out + o;
      u32 c = lane * 16;
      for (; c + 3 * 1024 + 16 <= len; c += 4096) {  // sixteen octets per lane, four loads in flight (eight: no faster)
        const K2U128 v0 = *(const K2U128*)(in + c), v1 = *(const K2U128*)(in + c + 1024);
        const K2U128 v2 = *(const K2U128*)(in + c + 2048), v3 = *(const K2U128*)(in + c + 3072);
        *(K2U128*)(out + c) = v0;
        *(K2U128*)(out + c + 1024) = v1;
        *(K2U128*)(out + c + 2048) = v2;
        *(K2U128*)(out + c + 3072) = v3;
      }
      for (; c < len; c += 1024) {
        if (c + 16 <= len) {
          *(K2U128*)(out + c) = *(const K2U128*)(in + c);
        } else {
          for (u32 k = c; k < len; k++) out[k] = in[k];
        }
      }
      at += 5 + len;
      o += len;
    }
    if (ok && P.format == 1 && at + 4 > P.in_len) ok = false;  // (a cut trailer: the general path says how much is missing)
    if (ok) {
      chain = true;
      if (lane == 0) {
        SegResult r{};
        r.status = SEG_FINAL;
        r.out_bytes = o;
        r.trailer_have = 2;
        if (P.format == 1) {
          r.trailer0 = ((u32)P.in[at] << 24) | ((u32)P.in[at + 1] << 16) | ((u32)P.in[at + 2] << 8) | P.in[at + 3];
          at += 4;
        }
        r.end_bit = at * 8;
        s_res = r;
      }
    }
  }
  // ---- (anything but a stored chain, whose octets cannot hold a flush point that counts) not this kernel's streams: flush points (the general path decodes their segments side by side and counts them),
  // and streams long enough for the block-start finder unless they begin with a stored block (raw deflate and zlib: the
  // first block header sits at a known place; a gzip header is parsed by K1, so a long gzip stream goes the general way)
  if (!chain && small_has_marker(P.in, P.in_len)) return leave(SMALL_FALLBACK, 0, 1);
  if (!chain && P.in_len >= P.find_min) {
    bool stored = false;
    if (P.format != 2) {
      const u64 hb = P.format == 1 ? 2 : 0;
      if (hb < P.in_len) stored = ((P.in[hb] >> 1) & 3) == 0;
    }
    if (!stored) return leave(SMALL_FALLBACK, 0, 2);
  }
  // ---- K1: the whole stream is one item for a gang of 64
  if (!chain) {
    K1gParams kp{};
    kp.in_base = P.in;
    kp.tok = P.tok;
    kp.runs = P.runs;
    kp.half = 1;
    kp.only_wide = 0;
    kp.items = &s_item;
    kp.res = &s_res;
    kp.markers = nullptr;
    kp.first_marker = s_fm;
    kp.hdr = nullptr;
    kp.hdr_lens = nullptr;
    kp.n_markers = 0;
    kp.n_items = 1;
    kp.ovl = 1024;
    kp.sub_min = KG_SUB_MIN;
    kp.wide_bits = 0;
    kp.resume_bit = 0;
    kp.cold = nullptr;  // (gangs of 64 keep their canonical lists in LDS)
    k1g_body<64>(kp, S.k1);
  }
  tbz_sync();
  const SegResult q = s_res;
  const bool container = P.format != 0;
  if (q.status != SEG_FINAL) return leave(SMALL_FALLBACK, 0, 3);
  if (q.max_deficit != 0 || q.out_bytes > P.out_cap || q.out_bytes > SMALL_MAX_OUT) return leave(SMALL_FALLBACK, 0, 4);
  if (container && q.trailer_have != 2) return leave(SMALL_FALLBACK, 0, 5);
  // ---- K2: one segment, one group, through the ring window
  const u32 n_out = (u32)q.out_bytes;
  if (q.tok_words) {
    Seg sg{};
    sg.tok = q.tok;
    sg.tok_words = q.tok_words;
    sg.out_bytes = q.out_bytes;
    sg.n_runs = q.n_runs;
    sg.run_first = 0;
    sg.runs = q.runs;
    sg.run0 = q.run0;
    Group g{};
    g.out_abs = 0;
    g.out_end = q.out_bytes;
    g.seg_first = 0;
    g.seg_count = 1;
    K2Params Q{};
    Q.in_base = P.in;
    Q.out_base = P.out;
    Q.n_groups = 1;
    k2_idt_init(S.k2.idt, 64);
    tbz_sync();
    K2Src src{S.k2.win, S.k2.idt, P.out, 0, 0};
    k2_body<K2Ring, K2_SPAN, false>(
        Q, 0, g, sg, S.k2.win, S.k2.tks, S.k2.rcache,
        [&](u64 pend, u32 rpos, u64 gpos, u32 dofs, u32 len, u32 dist) { k2_resolve<K2Ring>(src, pend, rpos, gpos, dofs, len, dist); },
        [](u64, u32) {});
  }
  // ---- checksum of what was written (zlib.lisp:97-102 / gzip.lisp:80-81), against the trailer K1 read
  u32 check = 0;
  if (container) {
    tbz_vm_drain();
    tbz_device_fence();  // the output was stored by this workgroup: read it back past the vector L1
    tbz_sync();
    if (P.format == 1) {
      u32 a = 0, b = 0;
      if (n_out) k4_adler_chunk(P.out, n_out, a, b);
      const u32 s1 = (1 + a) % ADLER_P, s2 = (n_out % ADLER_P + b) % ADLER_P;
      check = s1 | (s2 << 16);
    } else {
      for (u32 i = lane; i < CRC_X2N; i += 64) S.crc[i] = P.crc_tab[i];
      tbz_sync();
      const u32 raw = n_out ? k5_crc_chunk(S.crc, P.crc_tab, P.out, n_out) : 0u;
      check = (crc_mulmod(crc_pow_x8(P.crc_tab + CRC_X2N, n_out), 0xffffffffu) ^ raw) ^ 0xffffffffu;
    }
    if (check != q.trailer0) return leave(SMALL_FALLBACK, check, 6);  // (the general path reports the mismatch)
  }
  leave(SMALL_DONE, check, 0);
}


// ================================================================================================
// KX — tbz_ix_copy: batched segmented copy between device buffers (the seek index: capture the 32 KiB windows when an
// index is built, place each span's window in front of its output before a range decode, deliver the requested octets
// to the caller's buffer).  3bz has no counterpart (decompress-vector's :start / :end select INPUT, api.lisp:23-29).
// One workgroup of four waves per piece; the host cuts long records into pieces of at most IX_PIECE octets, so one
// long range is spread over the whole chip.  Source and destination alignment are arbitrary and independent:
//   head   the octets up to the destination's next 16-octet boundary, one per lane
//   body   16 octets per lane and step, one aligned 16-octet store.  Source 16-aligned at that point: one aligned
//          16-octet load.  Otherwise the two aligned 16-octet lines that hold the octets are loaded (the second is
//          the next lane's first: one HBM fetch, the other a hit) and realigned with v_alignbit over their eight words;
//          the misalignment is the same for every step of a piece, so the word selection is a wave-uniform switch
//          with constant register indices (no scratch)
//   tail   the last < 16 octets, one per lane
// A record's source must come from one of the engine's own buffers (16-aligned allocations with at least 16 octets of
// slack behind the last octet): the aligned lines the body loads may begin before the record and end behind it.
// Nothing outside [dst, dst + len) is written.
// ================================================================================================
struct IxRec {
  u64 src, dst;  // octet offsets in src_base / dst_base
  u64 len;
};
struct IxCopyParams {
  const u8* src_base;
  u8* dst_base;
  const IxRec* recs;
  u32 n_recs;
};
constexpr u32 IX_PIECE = 64u << 10;  // octets per workgroup: 16 steps of 256 lanes x 16 octets
constexpr u32 IX_THREADS = 256;

#define TBZ_IX_REALIGN(W0, W1, W2, W3, W4) \
  o.x = tbz_alignbit(W1, W0, sh);          \
  o.y = tbz_alignbit(W2, W1, sh);          \
  o.z = tbz_alignbit(W3, W2, sh);          \
  o.w = tbz_alignbit(W4, W3, sh);

TBZ_KERNEL_WG(256, 1) void tbz_ix_copy(IxCopyParams P) {
  const u32 r = tbz_block();
  if (r >= P.n_recs) return;
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const IxRec R = P.recs[r];
  const u8* TBZ_RESTRICT s = P.src_base + R.src;
  u8* TBZ_RESTRICT d = P.dst_base + R.dst;
  const u64 n = R.len;
  const u64 head = n < (u64)((0 - (uintptr_t)d) & 15) ? n : (u64)((0 - (uintptr_t)d) & 15);
  if (t < head) d[t] = s[t];
  const u64 units = (n - head) >> 4;
  const u8* sb = s + head;
  u8* db = d + head;
  const u32 k = (u32)((uintptr_t)sb & 15);  // (the same for every step: both sides advance by 16)
  if (k == 0) {
    for (u64 u = t; u < units; u += IX_THREADS) *(tbz_u32x4*)(db + u * 16) = *(const tbz_u32x4*)(sb + u * 16);
  } else {
    const u8* al = sb - k;
    const u32 sh = (k & 3) * 8;
    const u32 wo = k >> 2;
    for (u64 u = t; u < units; u += IX_THREADS) {
      const tbz_u32x4 a = *(const tbz_u32x4*)(al + u * 16);
      const tbz_u32x4 b = *(const tbz_u32x4*)(al + u * 16 + 16);
      tbz_u32x4 o;
      switch (wo) {
        case 0: TBZ_IX_REALIGN(a.x, a.y, a.z, a.w, b.x) break;
        case 1: TBZ_IX_REALIGN(a.y, a.z, a.w, b.x, b.y) break;
        case 2: TBZ_IX_REALIGN(a.z, a.w, b.x, b.y, b.z) break;
        default: TBZ_IX_REALIGN(a.w, b.x, b.y, b.z, b.w) break;
      }
      *(tbz_u32x4*)(db + u * 16) = o;
    }
  }
  const u64 done = head + units * 16;
  if (t < n - done) d[done + t] = s[done + t];
}
#undef TBZ_IX_REALIGN

// ================================================================================================
// KR — tbz_rec_count / tbz_rec_locate: records (the seek index's tbz_index_build_records, tbz_inflate_records*).  A
// record ends with one delimiter octet; the index keeps the number of delimiter octets in front of every point, so the
// interval that holds a record's end is known without decoding, and these two kernels do the rest over decoded octets
// in device memory: count the delimiter octets of pieces of at most IX_PIECE octets, and find the j-th of an interval.
// Both read the octets the way tbz_ix_copy's body does: whole aligned 16-octet lines around a piece (the source is one
// of the engine's own buffers), the octets of the first and the last line that lie outside the piece masked off.
// The per-octet test is exact: with x = word ^ (delim in every octet), ((x & 0x7f7f7f7f) + 0x7f7f7f7f) | x has an
// octet's top bit SET iff that octet of x is not zero — the add cannot carry out of an octet, so no octet's answer
// depends on its neighbour (the borrow-propagating (x - 0x01010101) & ~x & 0x80808080 reports 00 01 as two matches).
// ================================================================================================
struct RecPiece {
  u64 src;   // octet offset in src_base; any alignment
  u32 len;   // <= IX_PIECE
  u32 slot;  // counts[slot] receives the number of octets equal to delim
};
struct RecCountParams {
  const u8* src_base;
  const RecPiece* pieces;
  u32* counts;
  u32 n_pieces;
  u32 delim4;  // the delimiter in all four octets of a word
};
// one query: the interval lies at src_base + src, is len octets long, and the counts of its pieces (cut from its start,
// IX_PIECE octets each, the last one shorter) are counts[cnt0 ..].  out_pos[query] receives the offset in the interval of
// its j-th delimiter octet (0-based), or all ones if it holds fewer.
struct RecQuery {
  u64 src, len, j;
  u32 cnt0, pad;
};
struct RecLocateParams {
  const u8* src_base;
  const RecQuery* queries;
  const u32* counts;
  u64* out_pos;
  u32 n_queries;
  u32 delim4;
};
constexpr u64 REC_NONE = ~0ull;

// the top bit of every octet of w that equals the delimiter
TBZ_DEV u32 rec_match(u32 w, u32 delim4) {
  const u32 x = w ^ delim4;
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}
// all ones in the octets of a word whose positions pos .. pos + 3 lie in [0, n)
TBZ_DEV u32 rec_keep(i64 pos, i64 n) {
  const i64 lo = pos < 0 ? -pos : 0, hi = n - pos;  // octets [lo, hi) of the word
  if (lo >= 4 || hi <= lo) return 0u;
  const u32 above = 0xffffffffu << (8 * (u32)lo);
  return hi >= 4 ? above : above & (0xffffffffu >> (8 * (u32)(4 - hi)));
}
// matches in the aligned 16-octet line `u` of a piece of n octets that starts k octets (0..15) behind `al`
TBZ_DEV u32 rec_count_line(const u8* al, u32 u, u32 k, u32 n, u32 last, u32 delim4) {
  const tbz_u32x4 v = *(const tbz_u32x4*)(al + (u64)u * 16);
  u32 m0 = rec_match(v.x, delim4), m1 = rec_match(v.y, delim4), m2 = rec_match(v.z, delim4), m3 = rec_match(v.w, delim4);
  if (u == 0 || u == last) {  // (the only lines that can hold octets of other pieces)
    const i64 p = (i64)u * 16 - (i64)k;
    m0 &= rec_keep(p, n);
    m1 &= rec_keep(p + 4, n);
    m2 &= rec_keep(p + 8, n);
    m3 &= rec_keep(p + 12, n);
  }
  return tbz_popc64(((u64)m0 << 32) | m1) + tbz_popc64(((u64)m2 << 32) | m3);
}

TBZ_KERNEL_WG(256, 1) void tbz_rec_count(RecCountParams P) {
  TBZ_SHARED u32 s_wave[4];
  const u32 r = tbz_block();
  if (r >= P.n_pieces) return;
  const u32 w = tbz_wave(), t = w * 64 + tbz_lane();
  const RecPiece R = P.pieces[r];
  const u8* s = P.src_base + R.src;
  const u32 k = (u32)((uintptr_t)s & 15), n = R.len;
  const u8* al = s - k;
  const u32 lines = (k + n + 15) >> 4;  // (<= 4097)
  u32 c = 0;
  for (u32 u = t; u < lines; u += IX_THREADS) c += rec_count_line(al, u, k, n, lines - 1, P.delim4);
  c = tbz_wave_incl_scan_u32(c);
  if (tbz_lane() == 63) s_wave[w] = c;
  tbz_wg_barrier();
  if (t == 0) P.counts[R.slot] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

constexpr u32 REC_CHUNK = 64;  // octets a lane counts per round of the search inside a piece: four aligned lines

TBZ_KERNEL_WG(256, 1) void tbz_rec_locate(RecLocateParams P) {
  TBZ_SHARED u32 s_wave[2][4];
  TBZ_SHARED u32 s_hit[2];
  const u32 qi = tbz_block();
  if (qi >= P.n_queries) return;
  const u32 lane = tbz_lane(), w = tbz_wave(), t = w * 64 + lane;
  const RecQuery Q = P.queries[qi];
  // ---- the piece that holds delimiter j: every wave walks the interval's piece counts, 64 a step (the same values
  // in every wave: nothing to hand over)
  const u64 n_pieces = (Q.len + IX_PIECE - 1) / IX_PIECE;
  u64 before = 0, piece = REC_NONE;
  for (u64 base = 0; base < n_pieces; base += 64) {
    const u32 c = base + lane < n_pieces ? P.counts[Q.cnt0 + base + lane] : 0u;
    const u32 incl = tbz_wave_incl_scan_u32(c);  // (64 pieces hold at most 2^22 octets)
    const u64 here = tbz_ballot(before + incl > Q.j);
    if (here) {
      const u32 l = tbz_ffs64(here) - 1;
      piece = base + l;
      before += tbz_shfl(incl - c, (int)l);
      break;
    }
    before += tbz_shfl(incl, 63);
  }
  if (piece == REC_NONE) {
    if (t == 0) P.out_pos[qi] = REC_NONE;
    return;
  }
  // ---- inside the piece: rounds of 256 lanes x REC_CHUNK octets in octet order, a workgroup scan of the lanes' counts
  // per round; the lane whose chunk holds the octet names it, and a ballot over the chunk's 64 octets finds it
  const u8* s = P.src_base + Q.src + piece * IX_PIECE;
  const u64 left = Q.len - piece * IX_PIECE;
  const u32 n = left < IX_PIECE ? (u32)left : IX_PIECE;
  const u32 k = (u32)((uintptr_t)s & 15);
  const u8* al = s - k;
  const u32 lines = (k + n + 15) >> 4;
  const u32 chunks = (lines + 3) >> 2;  // (<= 1025)
  u32 want = (u32)(Q.j - before);       // ordinal inside the piece
  bool found = false;
  for (u32 c0 = 0; c0 < chunks; c0 += IX_THREADS) {
    const u32 ch = c0 + t;
    u32 c = 0;
    if (ch < chunks) {
#pragma unroll
      for (u32 i = 0; i < 4; i++)
        if (ch * 4 + i < lines) c += rec_count_line(al, ch * 4 + i, k, n, lines - 1, P.delim4);
    }
    const u32 incl = tbz_wave_incl_scan_u32(c);
    const u32 par = (c0 / IX_THREADS) & 1;  // (two sets of wave totals: a wave may be one round ahead of another)
    if (lane == 63) s_wave[par][w] = incl;
    tbz_wg_barrier();
    const u32 t0 = s_wave[par][0], t1 = s_wave[par][1], t2 = s_wave[par][2], t3 = s_wave[par][3];
    const u32 total = t0 + t1 + t2 + t3;
    if (want < total) {
      const u32 excl = incl - c + (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
      if (want >= excl && want < excl + c) {  // exactly one lane of the workgroup
        s_hit[0] = ch;
        s_hit[1] = want - excl;
      }
      found = true;
      break;
    }
    want -= total;
  }
  if (!found) {  // (the counts are of other octets than these: the caller compares them with the index first)
    if (t == 0) P.out_pos[qi] = REC_NONE;
    return;
  }
  tbz_wg_barrier();
  const u32 ch = s_hit[0], rank = s_hit[1];
  const i64 pos = (i64)ch * REC_CHUNK + lane - (i64)k;  // this lane's octet of the chunk, from the piece's start
  const bool in = pos >= 0 && pos < (i64)n;
  const u32 octet = in ? al[(u64)ch * REC_CHUNK + lane] : 0u;
  const bool hit = in && octet == (P.delim4 & 0xffu);
  const u64 hits = tbz_ballot(hit);
  if (w == 0 && hit && tbz_popc64(hits & ((1ull << lane) - 1)) == rank) P.out_pos[qi] = piece * IX_PIECE + (u64)pos;
}

// ================================================================================================
// KS — tbz_search_mark / tbz_search_emit: which records of a run hold a pattern (tbz_search_records*).  The run is
// whole records, decoded and checked, in the span scratch; the host has counted the delimiter octets of its pieces
// (tbz_rec_count) and prefix-summed them, so every piece knows the ordinal, within the run, of the record its first
// octet belongs to.  tbz_search_mark sets flags[ordinal of the record] = 1 for every occurrence of the pattern: one
// octet per record, every writer stores the same value and the store is idempotent, so there is no atomic and no
// bitmap word that two workgroups would have to share.  The host counts the set flags per piece of the flag array
// (tbz_rec_count again, "delimiter" 1), prefix-sums them, and tbz_search_emit writes first_record + index of every set
// flag to hits[its rank], ascending, as long as the rank is below the room left.
// Both read like tbz_rec_locate inside a piece: rounds of 256 lanes x REC_CHUNK octets in octet order, whole aligned
// 16-octet lines, the octets of the first and the last line outside the piece masked off, a workgroup scan of the
// lanes' counts per round with a carry across rounds.  A lane's chunk becomes two 64-bit masks (octets equal to the
// pattern's first octet: the candidates; delimiter octets), so a candidate's record is the carry plus the popcount of
// the delimiter mask in front of it.  Candidates are verified word by word against the pattern (eight words by value:
// constant indices, no scratch); a pattern whose first octet never occurs costs one read of the run, and one that is
// a candidate everywhere costs at most m compares per octet.  An occurrence may end in the next piece (the same
// buffer) but never at or behind the run's end: those octets are the next record's, or slack.  The host refuses
// patterns with a delimiter in front of their last octet, so an occurrence inside the run lies inside one record.
// ================================================================================================
struct SearchPiece {
  u64 src;   // octet offset in src_base (mark) / in the flag array (emit); any alignment
  u64 base;  // mark: ordinal in the run of the record of the piece's first octet; emit: set flags in front of the piece
  u32 len;   // <= IX_PIECE
  u32 pad;
};
struct SearchMarkParams {
  const u8* src_base;
  const SearchPiece* pieces;
  u64 end;     // offset in src_base of the octet behind the run's last
  u8* flags;   // one octet per record of the run, zeroed
  u32 n_pieces;
  u32 m;       // 1 .. 32
  u32 delim4;
  u32 pat[8];  // the pattern, little-endian words, zero behind its last octet
};
struct SearchEmitParams {
  const u8* flags;
  const SearchPiece* pieces;
  u64* hits;
  u64 first_record;  // the record of flags[0]
  u64 room;          // ranks below this are written
  u32 n_pieces;
  u32 pad;
};

// bit j: octet j of the word matched (rec_match's top bits, packed)
TBZ_DEV u32 search_bits4(u32 mm) {
  u32 x = mm >> 7;
  x |= x >> 7;
  x |= x >> 14;
  return x & 0xfu;
}
// one bit per octet of the aligned 16-octet line `u` of a piece (n octets, k behind `al`): equal to a4's octet / to b4's
TBZ_DEV void search_line(const u8* al, u32 u, u32 k, u32 n, u32 last, u32 a4, u32 b4, u32& ma, u32& mb) {
  const tbz_u32x4 v = *(const tbz_u32x4*)(al + (u64)u * 16);
  u32 a0 = rec_match(v.x, a4), a1 = rec_match(v.y, a4), a2 = rec_match(v.z, a4), a3 = rec_match(v.w, a4);
  u32 b0 = rec_match(v.x, b4), b1 = rec_match(v.y, b4), b2 = rec_match(v.z, b4), b3 = rec_match(v.w, b4);
  if (u == 0 || u == last) {
    const i64 p = (i64)u * 16 - (i64)k;
    const u32 k0 = rec_keep(p, n), k1 = rec_keep(p + 4, n), k2 = rec_keep(p + 8, n), k3 = rec_keep(p + 12, n);
    a0 &= k0; a1 &= k1; a2 &= k2; a3 &= k3;
    b0 &= k0; b1 &= k1; b2 &= k2; b3 &= k3;
  }
  ma = search_bits4(a0) | (search_bits4(a1) << 4) | (search_bits4(a2) << 8) | (search_bits4(a3) << 12);
  mb = search_bits4(b0) | (search_bits4(b1) << 4) | (search_bits4(b2) << 8) | (search_bits4(b3) << 12);
}
// ... of chunk `ch` (four lines): bit j is the octet at al + ch * REC_CHUNK + j
TBZ_DEV void search_chunk(const u8* al, u32 ch, u32 k, u32 n, u32 lines, u32 a4, u32 b4, u64& A, u64& B) {
  A = 0;
  B = 0;
#pragma unroll
  for (u32 i = 0; i < 4; i++)
    if (ch * 4 + i < lines) {
      u32 ma, mb;
      search_line(al, ch * 4 + i, k, n, lines - 1, a4, b4, ma, mb);
      A |= (u64)ma << (16 * i);
      B |= (u64)mb << (16 * i);
    }
}
// the workgroup's exclusive scan of c in lane order, and the total, over one set of wave totals
TBZ_DEV u32 search_wg_scan(u32 (*s_wave)[4], u32 par, u32 c, u32& total) {
  const u32 w = tbz_wave();
  const u32 incl = tbz_wave_incl_scan_u32(c);
  if (tbz_lane() == 63) s_wave[par][w] = incl;
  tbz_wg_barrier();
  const u32 t0 = s_wave[par][0], t1 = s_wave[par][1], t2 = s_wave[par][2], t3 = s_wave[par][3];
  total = t0 + t1 + t2 + t3;
  return incl - c + (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
}
// out[0 .. m) == pattern?  q + m lies within the run; the last word's octets behind m are read (the buffer's slack at
// most) and masked
TBZ_DEV bool search_verify(const u8* q, const u32 (&pat)[8], u32 m) {
  bool ok = true;
#pragma unroll
  for (u32 i = 0; i < 8; i++)
    if (ok && i * 4 < m) {
      const u8* p = q + i * 4;
      const u32 w = (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
      const u32 left = m - i * 4;
      const u32 keep = left >= 4 ? 0xffffffffu : (1u << (8 * left)) - 1u;
      ok = ((w ^ pat[i]) & keep) == 0;
    }
  return ok;
}

TBZ_KERNEL_WG(256, 1) void tbz_search_mark(SearchMarkParams P) {
  TBZ_SHARED u32 s_wave[2][4];
  const u32 r = tbz_block();
  if (r >= P.n_pieces) return;
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const SearchPiece R = P.pieces[r];
  const u8* s = P.src_base + R.src;
  const u32 k = (u32)((uintptr_t)s & 15), n = R.len;
  const u8* al = s - k;
  const u32 lines = (k + n + 15) >> 4;
  const u32 chunks = (lines + 3) >> 2;  // (<= 1025)
  const u32 first4 = (P.pat[0] & 0xffu) * 0x01010101u;
  const u64 al_off = R.src - k;  // `al` as an offset in src_base
  u64 carry = R.base;
  for (u32 c0 = 0; c0 < chunks; c0 += IX_THREADS) {
    const u32 ch = c0 + t;
    u64 cand = 0, dl = 0;
    if (ch < chunks) search_chunk(al, ch, k, n, lines, first4, P.delim4, cand, dl);
    u32 total;
    const u32 excl = search_wg_scan(s_wave, (c0 / IX_THREADS) & 1, tbz_popc64(dl), total);
    while (cand) {  // (lane-private: no collective inside)
      const u32 b = tbz_ffs64(cand) - 1;
      cand &= cand - 1;
      const u64 at = (u64)ch * REC_CHUNK + b;  // from `al`
      if (al_off + at + P.m <= P.end && search_verify(al + at, P.pat, P.m))
        P.flags[carry + excl + tbz_popc64(dl & ((1ull << b) - 1))] = 1;
    }
    carry += total;
  }
}

TBZ_KERNEL_WG(256, 1) void tbz_search_emit(SearchEmitParams P) {
  TBZ_SHARED u32 s_wave[2][4];
  const u32 r = tbz_block();
  if (r >= P.n_pieces) return;
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const SearchPiece R = P.pieces[r];
  const u8* s = P.flags + R.src;
  const u32 k = (u32)((uintptr_t)s & 15), n = R.len;
  const u8* al = s - k;
  const u32 lines = (k + n + 15) >> 4;
  const u32 chunks = (lines + 3) >> 2;
  u64 carry = R.base;
  for (u32 c0 = 0; c0 < chunks; c0 += IX_THREADS) {
    const u32 ch = c0 + t;
    u64 set = 0, same = 0;
    if (ch < chunks) search_chunk(al, ch, k, n, lines, 0x01010101u, 0x01010101u, set, same);
    u32 total;
    const u32 excl = search_wg_scan(s_wave, (c0 / IX_THREADS) & 1, tbz_popc64(set), total);
    u64 rank = carry + excl;
    while (set && rank < P.room) {
      const u32 b = tbz_ffs64(set) - 1;
      set &= set - 1;
      P.hits[rank++] = P.first_record + R.src + ((u64)ch * REC_CHUNK + b - k);
    }
    carry += total;
  }
}

// ================================================================================================
// KG — tbz_grep_bounds / _spans / _sum / _offs / _gather: the matching records' octets, packed (tbz_grep_records*).  They
// run behind KS in the same stage, while the run still lies in the span scratch, over the flags KS has set:
//   bounds   one more walk over the run's pieces (tbz_search_mark's walk: the delimiter ordinals carried across rounds).
//            A delimiter octet whose record or whose successor record is flagged stores the position behind it, from the
//            run's start, to ends[its ordinal]: one writer per entry, and no query per hit
//   spans    tbz_search_emit's walk over the flags: the hit of rank r starts at ends[record - 1] (the run's start for its
//            first record) and ends at ends[record] (the run's end for a last record without a delimiter), so
//            src[r] = where it lies in the scratch and len[r] = its octets, for the ranks below the room left
//   sum      the sum of len[] per chunk of GREP_CHUNK hits; the host reads the sums back and prefix-sums them, continuing
//            the previous passes' total — no workgroup waits for another
//   offs     len[] becomes, in place, the offset BEHIND each hit in the packed output: the chunk's base + a workgroup scan
//   gather   destination-centred.  A workgroup owns a tile of GREP_TILE destination octets, cut at 16-octet boundaries of
//            the destination ADDRESS; it finds the hits that reach into its tile by binary search in the offsets, and a
//            lane assembles one aligned 16-octet unit per step: if the unit lies inside one hit, from the five aligned
//            words that hold its source octets (v_alignbit; the source is an engine buffer with slack, as for tbz_ix_copy),
//            otherwise octet by octet across the hits it spans.  A whole unit is one 16-octet store; the units at the
//            edges of [lo, hi) and those cut by a hit that does not fit store their octets singly.  Hit j is copied iff
//            offs[j + 1] <= cap, so the cost follows the delivered octets and nothing outside [lo, hi) is written.
// ================================================================================================
struct GrepBoundsParams {
  const u8* src_base;
  const SearchPiece* pieces;  // the run's pieces, as tbz_search_mark got them
  const u8* flags;            // one octet per record of the run
  u64* ends;                  // one entry per delimiter octet of the run
  u64 run0;                   // offset in src_base of the run's first octet
  u64 n_records;
  u32 n_pieces;
  u32 delim4;
};
struct GrepSpansParams {
  const u8* flags;
  const SearchPiece* pieces;  // of the flag array, as tbz_search_emit got them
  const u64* ends;
  u64* src;                   // per rank: offset in the span scratch of the hit's first octet
  u64* len;                   // per rank: its octets
  u64 run0, run_len, n_records;
  u64 room;                   // ranks below this are written
  u32 n_pieces;
  u32 to_end;                 // the run's last record has no delimiter: it ends at the run's end
};
struct GrepScanParams {
  u64* vals;         // n lengths; tbz_grep_offs turns them into the offsets behind each
  u64* sums;         // tbz_grep_sum: per chunk
  const u64* bases;  // tbz_grep_offs: per chunk, the offset of its first hit
  u64 n;
};
struct GrepGatherParams {
  const u8* src_base;
  u8* dst;          // the caller's buffer
  const u64* offs;  // offs[j] .. offs[j + 1]: where hit j of this pass lies in dst; offs[0] == lo
  const u64* src;
  u64 n_hits;       // >= 1
  u64 lo, hi;       // the destination octets this pass may write; hi <= cap, hi <= offs[n_hits]
  u64 cap;
  u64 tile0;        // the first workgroup's tile, counted from the 16-aligned address at or below dst
  u32 n_tiles;
  u32 pad;
};
constexpr u32 GREP_PER_LANE = 8;
constexpr u32 GREP_CHUNK = IX_THREADS * GREP_PER_LANE;  // hits per workgroup of sum / offs
constexpr u32 GREP_TILE = 16u << 10;                    // destination octets per workgroup of gather: 4 steps

TBZ_KERNEL_WG(256, 1) void tbz_grep_bounds(GrepBoundsParams P) {
  TBZ_SHARED u32 s_wave[2][4];
  const u32 r = tbz_block();
  if (r >= P.n_pieces) return;
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const SearchPiece R = P.pieces[r];
  const u8* s = P.src_base + R.src;
  const u32 k = (u32)((uintptr_t)s & 15), n = R.len;
  const u8* al = s - k;
  const u32 lines = (k + n + 15) >> 4;
  const u32 chunks = (lines + 3) >> 2;
  const u64 al_rel = R.src - k - P.run0;  // `al` from the run's start (wraps for the first piece; the sums below do not)
  u64 carry = R.base;
  for (u32 c0 = 0; c0 < chunks; c0 += IX_THREADS) {
    const u32 ch = c0 + t;
    u64 same = 0, dl = 0;
    if (ch < chunks) search_chunk(al, ch, k, n, lines, P.delim4, P.delim4, same, dl);
    u32 total;
    const u32 excl = search_wg_scan(s_wave, (c0 / IX_THREADS) & 1, tbz_popc64(dl), total);
    u64 d = carry + excl;  // ordinal of this lane's first delimiter octet == the record it ends
    u32 mine = dl ? P.flags[d] : 0u;
    while (dl) {
      const u32 b = tbz_ffs64(dl) - 1;
      dl &= dl - 1;
      const u32 next = d + 1 < P.n_records ? P.flags[d + 1] : 0u;
      if (mine | next) P.ends[d] = al_rel + (u64)ch * REC_CHUNK + b + 1;
      mine = next;
      d++;
    }
    carry += total;
  }
}

TBZ_KERNEL_WG(256, 1) void tbz_grep_spans(GrepSpansParams P) {
  TBZ_SHARED u32 s_wave[2][4];
  const u32 r = tbz_block();
  if (r >= P.n_pieces) return;
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const SearchPiece R = P.pieces[r];
  const u8* s = P.flags + R.src;
  const u32 k = (u32)((uintptr_t)s & 15), n = R.len;
  const u8* al = s - k;
  const u32 lines = (k + n + 15) >> 4;
  const u32 chunks = (lines + 3) >> 2;
  u64 carry = R.base;
  for (u32 c0 = 0; c0 < chunks; c0 += IX_THREADS) {
    const u32 ch = c0 + t;
    u64 set = 0, same = 0;
    if (ch < chunks) search_chunk(al, ch, k, n, lines, 0x01010101u, 0x01010101u, set, same);
    u32 total;
    const u32 excl = search_wg_scan(s_wave, (c0 / IX_THREADS) & 1, tbz_popc64(set), total);
    u64 rank = carry + excl;
    while (set && rank < P.room) {
      const u32 b = tbz_ffs64(set) - 1;
      set &= set - 1;
      const u64 rec = R.src + ((u64)ch * REC_CHUNK + b - k);  // within the run
      const u64 from = rec ? P.ends[rec - 1] : 0;
      const u64 to = (P.to_end && rec + 1 == P.n_records) ? P.run_len : P.ends[rec];
      P.src[rank] = P.run0 + from;
      P.len[rank] = to - from;
      rank++;
    }
    carry += total;
  }
}

TBZ_DEV u64 grep_wave_incl_scan_u64(u64 x) {
  const u32 lane = tbz_lane();
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    const u64 y = tbz_shfl_up64(x, d);
    if (lane >= d) x += y;
  }
  return x;
}
// the workgroup's exclusive scan of c in lane order, and the total
TBZ_DEV u64 grep_wg_scan_u64(u64* s_wave, u64 c, u64& total) {
  const u32 w = tbz_wave();
  const u64 incl = grep_wave_incl_scan_u64(c);
  if (tbz_lane() == 63) s_wave[w] = incl;
  tbz_wg_barrier();
  const u64 t0 = s_wave[0], t1 = s_wave[1], t2 = s_wave[2], t3 = s_wave[3];
  total = t0 + t1 + t2 + t3;
  return incl - c + (w > 0 ? t0 : 0ull) + (w > 1 ? t1 : 0ull) + (w > 2 ? t2 : 0ull);
}

TBZ_KERNEL_WG(256, 1) void tbz_grep_sum(GrepScanParams P) {
  TBZ_SHARED u64 s_wave[4];
  const u32 r = tbz_block();
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const u64 at = (u64)r * GREP_CHUNK + (u64)t * GREP_PER_LANE;
  u64 c = 0;
#pragma unroll
  for (u32 i = 0; i < GREP_PER_LANE; i++)
    if (at + i < P.n) c += P.vals[at + i];
  u64 total;
  grep_wg_scan_u64(s_wave, c, total);
  if (t == 0) P.sums[r] = total;
}

TBZ_KERNEL_WG(256, 1) void tbz_grep_offs(GrepScanParams P) {
  TBZ_SHARED u64 s_wave[4];
  const u32 r = tbz_block();
  const u32 t = tbz_wave() * 64 + tbz_lane();
  const u64 at = (u64)r * GREP_CHUNK + (u64)t * GREP_PER_LANE;
  u64 v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0, v6 = 0, v7 = 0;
  if (at + 0 < P.n) v0 = P.vals[at + 0];
  if (at + 1 < P.n) v1 = P.vals[at + 1];
  if (at + 2 < P.n) v2 = P.vals[at + 2];
  if (at + 3 < P.n) v3 = P.vals[at + 3];
  if (at + 4 < P.n) v4 = P.vals[at + 4];
  if (at + 5 < P.n) v5 = P.vals[at + 5];
  if (at + 6 < P.n) v6 = P.vals[at + 6];
  if (at + 7 < P.n) v7 = P.vals[at + 7];
  v1 += v0; v2 += v1; v3 += v2; v4 += v3; v5 += v4; v6 += v5; v7 += v6;
  u64 total;
  const u64 base = P.bases[r] + grep_wg_scan_u64(s_wave, v7, total);
  if (at + 0 < P.n) P.vals[at + 0] = base + v0;
  if (at + 1 < P.n) P.vals[at + 1] = base + v1;
  if (at + 2 < P.n) P.vals[at + 2] = base + v2;
  if (at + 3 < P.n) P.vals[at + 3] = base + v3;
  if (at + 4 < P.n) P.vals[at + 4] = base + v4;
  if (at + 5 < P.n) P.vals[at + 5] = base + v5;
  if (at + 6 < P.n) P.vals[at + 6] = base + v6;
  if (at + 7 < P.n) P.vals[at + 7] = base + v7;
}

// the largest j in [lo, hi] with offs[j] <= pos (offs ascending, offs[lo] <= pos)
TBZ_DEV u64 grep_find(const u64* offs, u64 lo, u64 hi, u64 pos) {
  while (lo < hi) {
    const u64 mid = lo + (hi - lo + 1) / 2;
    if (offs[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

TBZ_KERNEL_WG(256, 1) void tbz_grep_gather(GrepGatherParams P) {
  const u32 r = tbz_block();
  if (r >= P.n_tiles) return;
  const u32 t = tbz_wave() * 64 + tbz_lane();
  // positions `g` count from the 16-aligned address at or below dst: g = destination offset + A
  const u64 A = (u64)((uintptr_t)P.dst & 15);
  const u64 g_lo = P.lo + A, g_hi = P.hi + A;
  const u64 t_lo = (P.tile0 + r) * GREP_TILE, t_hi = t_lo + GREP_TILE;
  const u64 ta = t_lo > g_lo ? t_lo : g_lo, te = t_hi < g_hi ? t_hi : g_hi;
  if (ta >= te) return;
  // the hits that reach into the tile (the same in every lane)
  const u64 j_first = grep_find(P.offs, 0, P.n_hits - 1, ta - A);
  const u64 j_last = grep_find(P.offs, j_first, P.n_hits - 1, te - 1 - A);
  for (u64 g = t_lo + (u64)t * 16; g < te; g += (u64)IX_THREADS * 16) {
    const u64 a = g > g_lo ? g : g_lo, e = g + 16 < g_hi ? g + 16 : g_hi;
    if (a >= e) continue;
    const u64 pa = a - A, pe = e - A;  // destination offsets of the unit's octets
    u64 j = grep_find(P.offs, j_first, j_last, pa);
    u64 oj = P.offs[j], oj1 = P.offs[j + 1], sj = P.src[j];
    if (oj1 > P.cap) continue;  // (nor does any later hit fit)
    if (e - a == 16 && oj1 >= pe) {  // a whole unit inside one hit
      const u8* s = P.src_base + sj + (pa - oj);
      const u32 sh = (u32)((uintptr_t)s & 3) * 8;
      const u32* q = (const u32*)(s - ((uintptr_t)s & 3));
      const u32 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
      tbz_u32x4 o;
      o.x = tbz_alignbit(w1, w0, sh);
      o.y = tbz_alignbit(w2, w1, sh);
      o.z = tbz_alignbit(w3, w2, sh);
      o.w = tbz_alignbit(w4, w3, sh);
      *(tbz_u32x4*)(P.dst + pa) = o;
      continue;
    }
    // across hits, or a unit cut by [lo, hi): octet i of the unit is destination offset g - A + i
    u32 x0 = 0, x1 = 0, x2 = 0, x3 = 0, have = 0;
    bool fits = true;
#pragma unroll
    for (u32 i = 0; i < 16; i++) {
      const u64 pos = g + i - A;  // (wraps in front of dst; such octets are outside [a, e))
      if (fits && g + i >= a && g + i < e) {
        while (pos >= oj1) {
          j++;
          oj = oj1;
          oj1 = P.offs[j + 1];
          sj = P.src[j];
        }
        fits = oj1 <= P.cap;
        if (fits) {
          const u32 v = (u32)P.src_base[sj + (pos - oj)] << (8 * (i & 3));
          if ((i >> 2) == 0) x0 |= v;
          if ((i >> 2) == 1) x1 |= v;
          if ((i >> 2) == 2) x2 |= v;
          if ((i >> 2) == 3) x3 |= v;
          have |= 1u << i;
        }
      }
    }
    if (have == 0xffffu) {
      tbz_u32x4 o;
      o.x = x0;
      o.y = x1;
      o.z = x2;
      o.w = x3;
      *(tbz_u32x4*)(P.dst + pa) = o;
    } else {
#pragma unroll
      for (u32 i = 0; i < 16; i++)
        if (have & (1u << i)) {
          const u32 w = (i >> 2) == 0 ? x0 : (i >> 2) == 1 ? x1 : (i >> 2) == 2 ? x2 : x3;
          P.dst[g + i - A] = (u8)(w >> (8 * (i & 3)));
        }
    }
  }
}

}  // namespace tbz
