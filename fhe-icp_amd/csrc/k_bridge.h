// LWE -> LWE bridge key switch of a key rotation: a big LWE
// (a, b) under the old big key becomes one under the new big key s',
//   out = (0, .., 0, b) - sum_i sum_l d_{i,l} * BK[i][l],
// BK[i][l] an LWE under s' (dimension kN) of the constant
// s_old[i] * 2^(64 - beta l), d_{i,.} the digits of a_i as k_pack_digits forms
// them. The sums are the i8 MFMA GEMM of the key switch (k_keyswitch_mfma<8, 1>
// on the bridge key's byte planes, k_ksk_to_i8 with R = 0: the key layout
// [i][l][kN+1] is the KSK's with n + 1 = kN + 1 columns, the last column block
// padded); its epilogue's last-column term carries b. This file holds what
// differs: the key generation, the digits with the body kept and rows read
// through a row map, and the copy back through that map.
// Row map (Q, B, B_old): compact row c = q * B_old + b, b < B_old, is row
// q * B + b of a query-major Q x B result (the old documents of every query).
// Part of libfheicp (one translation unit: fheicp.hip includes it).
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

// k_pack_digits with the body kept (body[c] = b_c: the GEMM's last-column
// term) and the input rows read through the row map. Same digits, tie coins
// and A-fragment layout [cb][kb][lane][16 B], K level-major; count = Q * B_old
// compact rows. Grid (big / 64, ceil(count / 16)), 256 threads; zero_n1 as in
// k_ks_digits (the compact output rows, for the split-K atomics).
__global__ void __launch_bounds__(256) k_bridge_digits(const u64* __restrict__ in, int64_t count, int64_t B,
                                                       int64_t B_old, int big, int beta, int levels, int KB,
                                                       uint32_t* __restrict__ D, u64* __restrict__ body, int zero_n1,
                                                       u64* __restrict__ zero_out) {
  const int t = threadIdx.x, cl = t >> 4, iq = t & 15;
  const int64_t cb = blockIdx.y, c = cb * 16 + cl;
  const int i0 = blockIdx.x * 64 + iq * 4;
  if (zero_n1 > 0) {
    const int per = (zero_n1 + (int)gridDim.x - 1) / (int)gridDim.x;
    for (int e = t; e < 16 * per; e += 256) {
      const int q = e / per, col = (int)blockIdx.x * per + (e - q * per);
      const int64_t cz = cb * 16 + q;
      if (cz < count && col < zero_n1) zero_out[(size_t)cz * zero_n1 + col] = 0;
    }
  }
  if (c >= count) return;
  const int64_t qi = c / B_old;
  const u64* src = in + (size_t)(qi * B + (c - qi * B_old)) * (big + 1);
  if (blockIdx.x == 0 && iq == 0) body[c] = src[big];
  const int prec = levels * beta;
  const u64 half = 1ull << (beta - 1), mask = (1ull << beta) - 1;
  uint32_t packed[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) packed[s] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u64 x = src[i0 + q];
    u64 r = ((x >> (63 - prec)) + 1) >> 1;
#pragma unroll
    for (int s = 0; s < 8; ++s) {  // LSB-first: digit s is level levels - 1 - s
      if (s >= levels) break;
      const u64 low = (r >> (s * beta)) & mask;
      const u64 coin = (x >> (62 - prec - s)) & 1;
      const int d = (low > half || (low == half && coin)) ? (int)low - (1 << beta) : (int)low;
      r -= (u64)(int64_t)d << (s * beta);
      packed[s] |= (uint32_t)(uint8_t)(int8_t)d << (8 * q);
    }
  }
  const int lane = cl + 16 * ((i0 >> 4) & 3);
  const int kbi = i0 >> 6, kbl = big >> 6;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    const int kb = (levels - 1 - s) * kbl + kbi;
    D[(((size_t)cb * KB + kb) * 64 + lane) * 4 + ((i0 & 15) >> 2)] = packed[s];
  }
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
