// Seeded evaluation keys: a key travels as the body of
// every row and the public mask key its masks came from; the importing
// context regenerates the masks into the standard-form buffers, after which
// the conversions to the FFT and byte-plane forms run unchanged.
//   GLWE-row keys (bsk, the gadgets' bsks, the packing key): row r is k mask
//     polynomials, words [0, N) of stream (tag, r k + c), and N body words:
//     k_expand_ggsw_seeded (k_private_seeded.h) with rows = all rows of the key;
//   LWE-row keys (ksk, bridge key): row r of n1 words is words [0, n1 - 1) of
//     stream (tag, r) and one body word: k_expand_lwe_rows_seeded below.
// Part of libfheicp (one translation unit: fheicp.hip includes it).
#pragma once

#include "common.h"

// One ChaCha block (8 mask words) per thread: thread e of the grid takes block
// e % bpr of row e / bpr, bpr = ceil((n1 - 1) / 8); the last block of a row is
// partly used when 8 does not divide n1 - 1, and its thread also places the
// body word. A row starts at byte 8 r n1, in general 8-byte aligned and no
// more (n = 64: 520-byte rows; the bridge key: kN + 1 words): 8-byte stores only.
__global__ void __launch_bounds__(256) k_expand_lwe_rows_seeded(ChaKey Km, uint32_t tag, const u64* __restrict__ body,
                                                                int64_t rows, int n1, u64* __restrict__ out) {
  const int n = n1 - 1, bpr = (n + 7) >> 3;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = e / bpr;
  if (row >= rows) return;
  const int blk = (int)(e - row * bpr);
  u64* dst = out + (size_t)row * n1;
  u64 w[8];
  stream_block(Km, tag, (u64)row, (uint32_t)blk, w);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int t = 8 * blk + q;
    if (t < n) dst[t] = w[q];
  }
  if (blk == bpr - 1) dst[n] = body[row];
}

// Bodies for export: words [off, off + len) of every row of n1 words, packed
// (off = kN, len = N for GLWE rows; off = n1 - 1, len = 1 for LWE rows).
__global__ void __launch_bounds__(256) k_gather_key_bodies(const u64* __restrict__ key, int64_t rows, int n1, int off,
                                                           int len, u64* __restrict__ body) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = e / len;
  if (row >= rows) return;
  const int t = (int)(e - row * len);
  body[e] = key[(size_t)row * n1 + off + t];
}
