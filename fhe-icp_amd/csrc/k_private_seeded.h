// Both-private search on seeded payloads: a document GLWE
// and a GGSW row travel and rest as their body polynomial alone; the k mask
// polynomials are words of ChaCha20 streams under a PUBLIC mask key that
// travels with the payload (the noise came from a secret key of the client's
// and is inside the body). Stream addressing is the full-form encryption's
// (k_encrypt_packed, k_encrypt_ggsw):
//   document GLWE g, component i < k:  word iN + t of (TAG_ENC_MASK, id0 + g),
//   GGSW row r = cL + l, component c': word t of (TAG_GGSW_MASK, id0 + r k + c').
// The document operands of the two products are made straight from the bodies
// (the masks exist in registers only); the queries, a few hundred KB with
// three consumers, are expanded once into a workspace. Part of libfheicp
// (fheicp.hip includes it after k_extprod_q.h).
#pragma once

#include "common.h"

// The 8 words [i0, i0 + 8) of document GLWE g's (k+1)N words, 8 | i0: one
// ChaCha block of the mask stream for a mask component, 8 body words from
// memory otherwise. 8 | N, so the 8 words never straddle the two sources.
__device__ __forceinline__ void seeded_glwe_words8(const ChaKey& Km, u64 id, const u64* __restrict__ body, int kN,
                                                   int i0, u64 x[8]) {
  if (i0 < kN) {
    stream_block(Km, TAG_ENC_MASK, id, (uint32_t)(i0 >> 3), x);
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = body[i0 - kN + q];
  }
}

// k_glwe_digits from seeded documents, byte for byte its operand. body:
// [count][N], document GLWE c under stream id id0 + c (modulo 2^64). A thread
// takes 8 consecutive coefficients, one ChaCha block, so that no block is
// computed twice: the two dwords of a level sit side by side in the lane's 16
// bytes and leave as one 8-byte store. 128 | n1, so a workgroup's threads all
// take the same branch of seeded_glwe_words8. Grid (n1 / 128, ceil(count / 16)),
// 256 threads; rows past count are left as the caller zeroed them.
__global__ void __launch_bounds__(256) k_glwe_digits_seeded(ChaKey Km, const u64* __restrict__ body, u64 id0,
                                                            int64_t count, int N, int k, int beta, int levels, int KB,
                                                            uint32_t* __restrict__ D) {
  const int t = threadIdx.x, cl = t >> 4, iq = t & 15;
  const int64_t cb = blockIdx.y, c = cb * 16 + cl;
  const int i0 = blockIdx.x * 128 + iq * 8;
  if (c >= count) return;
  const int n1 = (k + 1) * N;
  u64 x[8];
  seeded_glwe_words8(Km, id0 + (u64)c, body + (size_t)c * N, k * N, i0, x);
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) lo[s] = hi[s] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    glwe_word_digits(x[q], beta, levels, [&](int s, int d) { lo[s] |= (uint32_t)(uint8_t)(int8_t)d << (8 * q); });
    glwe_word_digits(x[4 + q], beta, levels, [&](int s, int d) { hi[s] |= (uint32_t)(uint8_t)(int8_t)d << (8 * q); });
  }
  const int lane = cl + 16 * ((i0 >> 4) & 3);
  const int kbi = i0 >> 6, kbl = n1 >> 6;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    const int kb = (levels - 1 - s) * kbl + kbi;
    // dword (i0 & 15) >> 2 is 0 or 2: an 8-byte aligned pair
    uint32_t* dst = D + (((size_t)cb * KB + kb) * 64 + lane) * 4 + ((i0 & 15) >> 2);
    *(u64*)dst = (u64)lo[s] | ((u64)hi[s] << 32);
  }
}

// k_glwe_digits_rev from seeded documents, byte for byte its operand: 8
// coefficients m0 .. m0 + 7 of (g, c) per thread, per level the 8 bytes at
// F[N - 8 - m0] (d reversed) and at F[2N - 8 - m0] (-d reversed), both 8-byte
// aligned (8 | N, 8 | xq_fstride). Grid (ceil(n1 / 2048), G), 256 threads; the
// caller zeroes the buffer.
__global__ void __launch_bounds__(256) k_glwe_digits_rev_seeded(ChaKey Km, const u64* __restrict__ body, u64 id0,
                                                                int N, int k, int beta, int levels,
                                                                uint8_t* __restrict__ F) {
  const int n1 = (k + 1) * N;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n1) return;
  const size_t g = blockIdx.y;
  const int c = i0 / N, m0 = i0 - c * N;
  u64 x[8];
  seeded_glwe_words8(Km, id0 + (u64)g, body + g * N, k * N, i0, x);
  u64 pos[8], neg[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) pos[s] = neg[s] = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q)
    glwe_word_digits(x[q], beta, levels, [&](int s, int d) {
      pos[s] |= (u64)(uint8_t)(int8_t)d << (8 * (7 - q));
      neg[s] |= (u64)(uint8_t)(int8_t)-d << (8 * (7 - q));
    });
  const size_t fs = xq_fstride(N);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    uint8_t* row = F + ((g * (k + 1) + c) * levels + (levels - 1 - s)) * fs;
    *(u64*)(row + (N - 8 - m0)) = pos[s];
    *(u64*)(row + (2 * N - 8 - m0)) = neg[s];
  }
}

// Bodies -> full form, for the queries (and for interop and tests, the
// documents): output row R of (k+1)N words is k mask polynomials from the
// streams and body row R. Item R / rows (a query; one for all documents) has
// the stream id base ids[item], or id_base where ids is null; row r = R % rows
// of it, component c', takes words [c' comp_blk 8, .. + N) of stream
// (tag, base + r row_ids + c' comp_ids):
//   GGSW queries: rows = (k+1) L, row_ids = k, comp_ids = 1, comp_blk = 0;
//   documents:    rows = count,   row_ids = 1, comp_ids = 0, comp_blk = N / 8.
// One workgroup per row, a ChaCha block (64 bytes of output) per thread and step.
__global__ void __launch_bounds__(256) k_expand_ggsw_seeded(ChaKey Km, uint32_t tag, const u64* __restrict__ body,
                                                            const u64* __restrict__ ids, u64 id_base, int64_t rows,
                                                            int row_ids, int comp_ids, int comp_blk, int N, int k,
                                                            u64* __restrict__ out) {
  const int64_t R = blockIdx.x, item = R / rows, r = R - item * rows;
  const u64 base = (ids ? ids[item] : id_base) + (u64)r * (u64)row_ids;
  u64* o = out + (size_t)R * (k + 1) * N;
  const int bpc = N >> 3;  // blocks per component
  for (int blk = threadIdx.x; blk < k * bpc; blk += 256) {
    const int cp = blk / bpc, b = blk - cp * bpc;
    u64 w[8];
    stream_block(Km, tag, base + (u64)(cp * comp_ids), (uint32_t)(cp * comp_blk + b), w);
#pragma unroll
    for (int q = 0; q < 8; ++q) o[(size_t)cp * N + 8 * b + q] = w[q];
  }
  const u64* src = body + (size_t)R * N;
  for (int t = threadIdx.x; t < N; t += 256) o[(size_t)k * N + t] = src[t];
}
