// LWE -> LWE bridge key switch of a key rotation: a big LWE
// (a, b) under the old big key becomes one under the new big key s',
//   out = (0, .., 0, b) - sum_i sum_l d_{i,l} * BK[i][l],
// BK[i][l] an LWE under s' (dimension kN) of the constant
// s_old[i] * 2^(64 - beta l), d_{i,.} the digits of a_i as k_pack_digits forms
// them. The sums are the i8 MFMA GEMM of the key switch (k_keyswitch_mfma<8, 1>
// on the bridge key's byte planes, k_ksk_to_i8 with R = 0: the key layout
// [i][l][kN+1] is the KSK's with n + 1 = kN + 1 columns, the last column block
// padded); its epilogue's last-column term carries b. This file holds what
// differs: the key generation, the digits (wide_digits_group, k_pack.h) with
// the body kept and rows read through a row map, and the copy back through
// that map, in two forms.
// Row map (Q, B, B_old), one key: compact row c = q * B_old + b, b < B_old, is
// row q * B + b of a query-major Q x B result (the old documents of every
// query). k_bridge_digits / k_bridge_scatter; the GEMM is k_keyswitch_mfma.
// Segments, a key each: a segment is the n documents
// doc0 .. doc0 + n - 1 of every query of one query-major Q x B result that
// begins at row row0 of the buffer (one old key generation of a context,
// row0 = 0, or of a tenant of a group, row0 its first padded row). Its Q n
// compact rows are start .. start + Q n - 1, compact row start + q n + j
// standing for buffer row row0 + q B + doc0 + j; the segments follow each
// other unpadded. A segment owns ceil(rows / 128) ciphertext blocks and
// ceil(rows / 16) digit groups of its own (KsGrpBlock's convention with
// "tenant" = segment; k_ks_grp_tables builds the block table from starts |
// ends), so a 128-row workgroup never straddles two segments. The host writes
// starts | ends | the segment records | the key table in stream order
// (store_words); the GEMM is k_keyswitch_mfma_grp<8, 1> with n1 = kN + 1,
// R = 0 and the segments' byte planes in its key table. Every table read is at
// a workgroup-uniform address (scalar loads). Rows that belong to no segment
// (current-key rows, padding, tenants that sit out) are neither read nor
// written. k_bridge_digits_seg / k_bridge_scatter_seg.
// Part of libfheicp (one translation unit: fheicp.hip includes it after
// k_ks_grp.h and k_pack.h).
#pragma once

#include "common.h"

// One workgroup per bridge-key row (i, l): LWE_{s'}(s_old[i] * 2^(64 - (l+1) beta)).
// Rows as k_keygen_ksk's: masks from stream (TAG_BRIDGE_MASK, row), the noise
// from word 0 of (TAG_BRIDGE_NOISE, row), body = sum_t a_t s'_t + e + message.
// Masks under the mask key Km, noise under the noise key Kn.
__global__ void __launch_bounds__(256) k_keygen_bridge(ChaKey Km, ChaKey Kn, int big, int L, int beta, int noise_bits,
                                                       const u64* __restrict__ s_new, const u64* __restrict__ s_old,
                                                       u64* __restrict__ bk) {
  __shared__ u64 red[4];
  const int row = blockIdx.x;  // i * L + l
  const int i = row / L, l = row % L;
  u64* dst = bk + (size_t)row * (big + 1);
  u64 part = 0;
  for (int blk = threadIdx.x; blk < big / 8; blk += 256) {  // big % 64 == 0
    u64 w[8];
    stream_block(Km, TAG_BRIDGE_MASK, (u64)row, (uint32_t)blk, w);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = 8 * blk + q;
      dst[t] = w[q];
      if (s_new[t]) part += w[q];
    }
  }
  const u64 s = block_sum_u64<256>(part, red);
  if (threadIdx.x == 0) {
    u64 b = s + (u64)tuniform(stream_word(Kn, TAG_BRIDGE_NOISE, (u64)row, 0), noise_bits);
    if (s_old[i]) b += 1ull << (64 - (l + 1) * beta);
    dst[big] = b;
  }
}

// The row map's digits: wide_digits_group with the body kept (body[c] = b_c:
// the GEMM's last-column term) and the input rows read through the row map;
// count = Q * B_old compact rows. Grid (big / 64, ceil(count / 16)), 256
// threads; zero_n1 as in k_ks_digits (the compact output rows, for the split-K
// atomics).
__global__ void __launch_bounds__(256) k_bridge_digits(const u64* __restrict__ in, int64_t count, int64_t B,
                                                       int64_t B_old, int big, int beta, int levels, int KB,
                                                       uint32_t* __restrict__ D, u64* __restrict__ body, int zero_n1,
                                                       u64* __restrict__ zero_out) {
  wide_digits_group((int64_t)blockIdx.y * 16, count, blockIdx.y,
                    [&](int64_t c) {
                      const int64_t qi = c / B_old;
                      return in + (size_t)(qi * B + (c - qi * B_old)) * (big + 1);
                    },
                    true, big, beta, levels, KB, D, body, zero_n1, zero_out);
}

// The GEMM's compact rows back to their places: out row q * B + b takes
// compact row q * B_old + b, n1 = kN + 1 words. Grid (count, ceil(n1 / 256)).
__global__ void __launch_bounds__(256) k_bridge_scatter(const u64* __restrict__ M, int64_t count, int64_t B,
                                                        int64_t B_old, int n1, u64* __restrict__ out) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  const int64_t c = blockIdx.x;
  if (col >= n1 || c >= count) return;
  const int64_t qi = c / B_old;
  out[(size_t)(qi * B + (c - qi * B_old)) * n1 + col] = M[(size_t)c * n1 + col];
}

struct BridgeSeg {
  int64_t start;  // first compact row of the segment
  int64_t n;      // documents of the segment; it holds Q n rows
  int64_t doc0;   // its first document among the result's B
  int64_t B;      // the result's documents: it is query-major Q x B
  int64_t row0;   // the result's first row of the buffer
};
#define BRIDGE_SEG_WORDS 5  // a record as the host stores it, in u64 words
static_assert(sizeof(BridgeSeg) == 8 * BRIDGE_SEG_WORDS, "BridgeSeg is five words");

// the buffer row of compact row c of segment s (c within the segment)
__device__ __forceinline__ int64_t bridge_seg_row(const BridgeSeg& s, int64_t c) {
  const int64_t r = c - s.start, qi = r / s.n;
  return s.row0 + qi * s.B + s.doc0 + (r - qi * s.n);
}

// The segments' digits: grid (big / 64, 8 * blocks), 256 threads; block y
// forms digit group y & 7 of ciphertext block y >> 3, the body kept (body[c],
// c the compact row), the source row through the block's segment record. A
// digit group past the segment's rows does not exist: nothing is read or
// written for it.
__global__ void __launch_bounds__(256) k_bridge_digits_seg(const u64* __restrict__ in,
                                                           const KsGrpBlock* __restrict__ blk,
                                                           const BridgeSeg* __restrict__ seg, int big, int beta,
                                                           int levels, int KB, uint32_t* __restrict__ D,
                                                           u64* __restrict__ body, int zero_n1,
                                                           u64* __restrict__ zero_out) {
  const KsGrpBlock e = blk[blockIdx.y >> 3];
  const int j = blockIdx.y & 7;
  const int64_t c0 = e.row0 + (int64_t)j * 16;  // the group's first compact row
  if (c0 >= e.end) return;
  const BridgeSeg sg = seg[e.tenant];
  wide_digits_group(c0, e.end, (size_t)e.dg0 + j,  // the digit group among all segments'
                    [&](int64_t c) { return in + (size_t)bridge_seg_row(sg, c) * (big + 1); }, true, big, beta,
                    levels, KB, D, body, zero_n1, zero_out);
}

// The GEMM's compact rows back to their places in the buffer: grid
// (8 * blocks, ceil(n1 / 256)); block x copies the (at most 16) rows of digit
// group x & 7 of ciphertext block x >> 3.
__global__ void __launch_bounds__(256) k_bridge_scatter_seg(const u64* __restrict__ M,
                                                            const KsGrpBlock* __restrict__ blk,
                                                            const BridgeSeg* __restrict__ seg, int n1,
                                                            u64* __restrict__ out) {
  const KsGrpBlock e = blk[blockIdx.x >> 3];
  const int64_t c0 = e.row0 + (int64_t)(blockIdx.x & 7) * 16;
  if (c0 >= e.end) return;
  const BridgeSeg sg = seg[e.tenant];
  const int col = blockIdx.y * 256 + threadIdx.x;
  if (col >= n1) return;
  const int64_t c1 = c0 + 16 < e.end ? c0 + 16 : e.end;
  for (int64_t c = c0; c < c1; ++c) out[(size_t)bridge_seg_row(sg, c) * n1 + col] = M[(size_t)c * n1 + col];
}
