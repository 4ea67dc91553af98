// Both-private search: a GGSW-encrypted query against
// GLWE-encrypted documents, as one exact external product modulo 2^64,
//   out_g = sum_{c <= k} sum_{l <= L} d_{g,c,l}(X) * Row(c, l)      (negacyclic),
// d_{g,c,.} the key switch's balanced digits with tie coins of component c
// (masks and body alike) of document GLWE g, Row(c, l) the query's GGSW rows.
// Written as a GEMM [G x (k+1)N L] . [(k+1)N L x (k+1)N] it is the packing key
// switch's (k_keyswitch_mfma<8, 1>, K level-major) with (k+1)N input words
// instead of kN and the negacyclic Toeplitz expansion of the rows as the key:
//   T[l (k+1)N + cN + u][c' N + t] = +-Row(c, l)[c'][(t - u) mod N], minus when t < u.
// The kernel computes body - D . K8, so the planes hold -T and the body is 0.
// This file holds what differs: the GGSW encryption of the sparse query
// polynomial, the documents' digits, the Toeplitz byte planes and the slot
// extraction. Part of libfheicp (one translation unit: fheicp.hip includes it
// after k_server.h, whose v4i and fragment layouts it shares).
#pragma once

#include "common.h"

// One workgroup per GGSW row (c, l), row = c L + l: a GLWE encryption under
// the big key (k polynomials S_c) of
//   Q 2^(64 - (l+1) beta)          for c = k,
//   -S_c Q 2^(64 - (l+1) beta)     for c < k,
// Q = sum_{j < D} W_j X^-j = W_0 - sum_{j >= 1} W_j X^(N-j) (plain integers,
// D <= N). Rows as k_keygen_pack's: masks from stream (TAG_GGSW_MASK,
// id0 + row k + c'), noise from (TAG_GGSW_NOISE, id0 + row), body = sum_c'
// A_c' S_c' + E + message. (S_c X^-j)[t] = S_c[t + j], or -S_c[t + j - N] past
// the end. Layout [c][l][component][coef]. The masks come from the key Km and
// the noise from Kn: one secret key twice for the full form, a public mask
// key and a secret noise key for the seeded form, which
// stores the bodies alone, [c][l][coef] (body_only).
__global__ void __launch_bounds__(256) k_encrypt_ggsw(ChaKey Km, ChaKey Kn, int N, int k, int L, int beta,
                                                      int noise_bits, const u64* __restrict__ s_big,
                                                      const int64_t* __restrict__ W, int D, u64 id0,
                                                      u64* __restrict__ ggsw, int body_only) {
  extern __shared__ u64 shm[];
  u64* A = shm;                                  // N
  unsigned char* S = (unsigned char*)(shm + N);  // N
  const int row = blockIdx.x;  // c * L + l
  const int c = row / L, l = row % L;
  u64* dst = ggsw + (size_t)row * (k + 1) * N;
  u64* bdst = body_only ? ggsw + (size_t)row * N : dst + (size_t)k * N;
  constexpr int MAXC = 8;  // N <= 2048 -> 8 coefficients per thread
  u64 body[MAXC];
  const int per = N / 256;
  for (int q = 0; q < per; ++q) body[q] = 0;
  for (int cc = 0; cc < k; ++cc) {
    const u64 sid = id0 + (u64)row * k + cc;
    for (int blk = threadIdx.x; blk < N / 8; blk += 256) {
      u64 w[8];
      stream_block(Km, TAG_GGSW_MASK, sid, (uint32_t)blk, w);
#pragma unroll
      for (int q = 0; q < 8; ++q) A[8 * blk + q] = w[q];
      if (!body_only) {
#pragma unroll
        for (int q = 0; q < 8; ++q) dst[(size_t)cc * N + 8 * blk + q] = w[q];
      }
    }
    for (int t = threadIdx.x; t < N; t += 256) S[t] = (unsigned char)s_big[(size_t)cc * N + t];
    __syncthreads();
    for (int v = 0; v < N; ++v) {
      if (!S[v]) continue;  // uniform across the block
      for (int q = 0; q < per; ++q) {
        const int t = threadIdx.x + 256 * q;
        body[q] += (t >= v) ? A[t - v] : (u64)0 - A[t - v + N];
      }
    }
    __syncthreads();
  }
  const int sh = 64 - (l + 1) * beta;
  for (int q = 0; q < per; ++q) {
    const int t = threadIdx.x + 256 * q;
    u64 m = 0;
    if (c == k) {
      if (t == 0) m = (u64)W[0];
      else if (N - t < D) m = (u64)0 - (u64)W[N - t];
    } else {
      const u64* Sc = s_big + (size_t)c * N;
      for (int j = 0; j < D; ++j) {
        const int i = t + j;
        const u64 wj = (u64)W[j];
        if (i < N) m -= Sc[i] ? wj : (u64)0;
        else m += Sc[i - N] ? wj : (u64)0;
      }
    }
    bdst[t] =
        body[q] + (m << sh) + (u64)tuniform(stream_word(Kn, TAG_GGSW_NOISE, id0 + (u64)row, (u64)t), noise_bits);
  }
}

// The key switch's balanced digits with tie coins of one document word,
// LSB-first (digit s is level levels - 1 - s), handed to put(s, d): the one
// digit code of the document operands here, in k_extprod_q.h and in
// k_private_seeded.h.
template <typename Put>
__device__ __forceinline__ void glwe_word_digits(u64 x, int beta, int levels, Put&& put) {
  const int prec = levels * beta;
  const u64 half = 1ull << (beta - 1), mask = (1ull << beta) - 1;
  u64 r = ((x >> (63 - prec)) + 1) >> 1;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    const u64 low = (r >> (s * beta)) & mask;
    const u64 coin = (x >> (62 - prec - s)) & 1;
    const int d = (low > half || (low == half && coin)) ? (int)low - (1 << beta) : (int)low;
    r -= (u64)(int64_t)d << (s * beta);
    put(s, d);
  }
}

// k_pack_digits on whole GLWEs: zero-mean digits of all n1 = (k+1)N words
// (row stride n1, no body column) in A-fragment order [cb][kb][lane][16 B],
// K level-major (k = l n1 + i). Runs once per resident corpus. Grid
// (n1 / 64, ceil(count / 16)), 256 threads; rows past count are left as the
// caller zeroed them.
__global__ void __launch_bounds__(256) k_glwe_digits(const u64* __restrict__ in, int64_t count, int n1, int beta,
                                                     int levels, int KB, uint32_t* __restrict__ D) {
  const int t = threadIdx.x, cl = t >> 4, iq = t & 15;
  const int64_t cb = blockIdx.y, c = cb * 16 + cl;
  const int i0 = blockIdx.x * 64 + iq * 4;
  if (c >= count) return;
  const u64* src = in + (size_t)c * n1;
  uint32_t packed[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) packed[s] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    glwe_word_digits(src[i0 + q], beta, levels,
                     [&](int s, int d) { packed[s] |= (uint32_t)(uint8_t)(int8_t)d << (8 * q); });
  const int lane = cl + 16 * ((i0 >> 4) & 3);
  const int kbi = i0 >> 6, kbl = n1 >> 6;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    const int kb = (levels - 1 - s) * kbl + kbi;
    D[(((size_t)cb * KB + kb) * 64 + lane) * 4 + ((i0 & 15) >> 2)] = packed[s];
  }
}

// The GEMM's right operand: the 8 byte planes of -T in B-fragment order
// [kb][nb][q][lane][16 B] (as k_ksk_to_i8 / k_query_planes). One wave
// (= workgroup) per fragment (kb, nb), one thread per fragment lane: lane l
// holds column 16 nb + (l & 15) = c' N + t and rows 64 kb + 16 (l >> 4) + j =
// l' n1 + c N + u0 + j in byte j. 16 | N, so the 16 rows share (l', c) and the
// lane reads Row(c, l')[c'][(t - u0 - j) mod N], 16 consecutive words
// downwards with one wrap at most; the GGSW (a few hundred KB) stays in L2.
// Grid KB * NB, KB = n1 L / 64, NB = n1 / 16.
__global__ void __launch_bounds__(64) k_extprod_planes(const u64* __restrict__ ggsw, int N, int k, int L, int NB,
                                                       v4i* __restrict__ out) {
  const int lane = threadIdx.x, f = blockIdx.x;
  const int kb = f / NB, nb = f - kb * NB;
  const int n1 = (k + 1) * N;
  const int col = nb * 16 + (lane & 15);
  const int cp = col / N, t = col - cp * N;
  const int r0 = kb * 64 + 16 * (lane >> 4);
  const int lv = r0 / n1, i = r0 - lv * n1;
  const int c = i / N, u0 = i - c * N;
  const u64* row = ggsw + (((size_t)c * L + lv) * (k + 1) + cp) * N;
  u64 xs[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int d = t - u0 - j;  // in (-N, N)
    xs[j] = d >= 0 ? (u64)0 - row[d] : row[d + N];  // -T: T is -row past the wrap
  }
  byte_planes16_store(true, [&](int j) { return xs[j]; }, out + (size_t)f * 8 * 64 + lane);
}

// Sample extraction of the slot at coefficient p of one GLWE src ((k+1) N
// words, a row of a GEMM result): word col <= kN of the big LWE (kN + 1 words)
// fhe_sign_batch and fhe_pack_batch take,
//   a_{cN + u} = A_c[p - u] for u <= p, -A_c[p - u + N] otherwise; b = B[p] + cst,
// cst already scaled to the encoding. The one extraction of the four extract
// kernels (here, k_extprod_q.h, k_extprod_grp.h), which differ in how a row
// finds its GLWE and its constant and in where it writes.
__device__ __forceinline__ u64 xq_extract_word(const u64* __restrict__ src, int p, int col, int N, int k, u64 cst) {
  if (col == k * N) return src[(size_t)k * N + p] + cst;
  const int c = col / N, u = col - c * N;
  return u <= p ? src[(size_t)c * N + p - u] : (u64)0 - src[(size_t)c * N + p - u + N];
}

// One slot per document: document b sits in GLWE g = b / S at coefficient
// p = (b % S) D of M (the GEMM's G x (k+1)N result). Grid (B, ceil((kN + 1) / 256)).
__global__ void __launch_bounds__(256) k_extprod_extract(const u64* __restrict__ M, int S, int D, int N, int k,
                                                         u64 cst_scaled, u64* __restrict__ out) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  const int64_t b = blockIdx.x;
  const int big = k * N;
  if (col > big) return;
  const int64_t g = b / S;
  const int p = (int)(b - g * S) * D;
  out[(size_t)b * (big + 1) + col] = xq_extract_word(M + (size_t)g * (k + 1) * N, p, col, N, k, cst_scaled);
}
