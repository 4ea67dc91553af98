// LWE -> GLWE packing key switch: up to N big LWEs folded
// into one GLWE under the big key,
//   out = sum_j X^j * [ (0, .., 0, b_j) - sum_i sum_{l <= L'} d_{j,i,l} * PK[i][l] ],
// PK[i][l] a GLWE encryption of the constant s_big[i] * 2^(64 - beta l).
// The inner sums are the i8 MFMA GEMM of the key switch (k_keyswitch_mfma<8, 1>
// on the packing key's byte planes, k_ksk_to_i8 with R = 0: the key layout
// [i][l][(k+1)N] is the KSK's with n + 1 = (k+1)N columns); this file holds
// what differs: digits past 32 bits (wide_digits_group, the bridge's too),
// the key generation, the negacyclic rotation-and-sum and the packed
// decryption.
// Part of libfheicp (one translation unit: fheicp.hip includes it).
#pragma once

#include "common.h"

// One workgroup per packing-key row (i, l): GLWE_S(s_big[i] * 2^(64 - (l+1) beta))
// as a constant polynomial, S the big key read as k polynomials. Rows as
// k_keygen_bsk's: masks from stream (tag_mask, row * k + c), noise from
// (tag_noise, row), body = sum_c A_c * S_c (negacyclic, binary S) + E + message.
// Masks under the mask key Km, noise under the noise key Kn.
__global__ void __launch_bounds__(256) k_keygen_pack(ChaKey Km, ChaKey Kn, int N, int k, int L, int beta, int noise_bits,
                                                     const u64* __restrict__ s_big, u64* __restrict__ pk) {
  extern __shared__ u64 shm[];
  u64* A = shm;                                  // N
  unsigned char* S = (unsigned char*)(shm + N);  // N
  const int row = blockIdx.x;  // i * L + l
  const int i = row / L, l = row % L;
  u64* dst = pk + (size_t)row * (k + 1) * N;
  constexpr int MAXC = 8;  // N <= 2048 -> 8 coefficients per thread
  u64 body[MAXC];
  const int per = N / 256;
  for (int q = 0; q < per; ++q) body[q] = 0;
  for (int c = 0; c < k; ++c) {
    const u64 sid = (u64)row * k + c;
    for (int blk = threadIdx.x; blk < N / 8; blk += 256) {
      u64 w[8];
      stream_block(Km, TAG_PACK_MASK, sid, (uint32_t)blk, w);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        A[8 * blk + q] = w[q];
        dst[(size_t)c * N + 8 * blk + q] = w[q];
      }
    }
    for (int t = threadIdx.x; t < N; t += 256) S[t] = (unsigned char)s_big[(size_t)c * N + t];
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
  for (int q = 0; q < per; ++q) {
    const int t = threadIdx.x + 256 * q;
    u64 b = body[q] + (u64)tuniform(stream_word(Kn, TAG_PACK_NOISE, (u64)row, (u64)t), noise_bits);
    if (t == 0 && s_big[i]) b += 1ull << (64 - (l + 1) * beta);
    dst[(size_t)k * N + t] = b;
  }
}

// k_ks_digits for gadgets up to beta * levels = 48 (the rounded value in 64
// bits; k_ks_digits keeps it in 32): zero-mean digits of the mask words in
// A-fragment order [dg][kb][lane][16 B], K level-major. No shift. The tie coin
// of digit s (LSB first) is input bit 62 - prec - s, an input bit for every
// s < levels when prec + levels <= 62.
// wide_digits_group is one workgroup's work (256 threads, 64 mask words of 16
// rows; blockIdx.x the word block of big / 64) on one digit group: the compact
// rows c0 .. min(c0 + 16, end) - 1, digit group dg of D. row(c) is the source
// row of compact row c (big + 1 words); body[c] (the GEMM's last-column term)
// takes that row's body when keep_body, else 0. With zero_n1 > 0 the group's
// rows of zero_out are zeroed as in k_ks_digits, for the split-K atomics.
// Shared by k_pack_digits and the bridge's digit kernels (k_bridge.h).
template <typename Row>
__device__ __forceinline__ void wide_digits_group(int64_t c0, int64_t end, size_t dg, Row&& row, bool keep_body,
                                                  int big, int beta, int levels, int KB, uint32_t* __restrict__ D,
                                                  u64* __restrict__ body, int zero_n1, u64* __restrict__ zero_out) {
  const int t = threadIdx.x, cl = t >> 4, iq = t & 15;
  const int64_t c = c0 + cl;
  const int i0 = blockIdx.x * 64 + iq * 4;
  if (zero_n1 > 0) {
    const int per = (zero_n1 + (int)gridDim.x - 1) / (int)gridDim.x;
    for (int e = t; e < 16 * per; e += 256) {
      const int q = e / per, col = (int)blockIdx.x * per + (e - q * per);
      const int64_t cz = c0 + q;
      if (cz < end && col < zero_n1) zero_out[(size_t)cz * zero_n1 + col] = 0;
    }
  }
  if (c >= end) return;
  const u64* src = row(c);
  if (blockIdx.x == 0 && iq == 0) body[c] = keep_body ? src[big] : 0;
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
    D[((dg * KB + kb) * 64 + lane) * 4 + ((i0 & 15) >> 2)] = packed[s];
  }
}
// The packing's digits: row c of `in` as it stands and no body (the rotation
// adds b_j where X^j puts it). Grid (big / 64, ceil(count / 16)), 256 threads.
__global__ void __launch_bounds__(256) k_pack_digits(const u64* __restrict__ in, int64_t count, int big, int beta,
                                                     int levels, int KB, uint32_t* __restrict__ D,
                                                     u64* __restrict__ body, int zero_n1, u64* __restrict__ zero_out) {
  wide_digits_group((int64_t)blockIdx.y * 16, count, blockIdx.y,
                    [&](int64_t c) { return in + (size_t)c * (big + 1); }, false, big, beta, levels, KB, D, body,
                    zero_n1, zero_out);
}

// out[g][c][t] += sum_j +-M[gN + j][c][(t - j) mod N] (minus when t < j: X^N =
// -1), plus b_{gN + t} on the body component: GLWE g takes inputs gN .. gN +
// cnt - 1. M is the GEMM's count x (k+1)N result, ct the packed LWEs (their
// bodies). A workgroup sums PK_JC consecutive j for 256 coefficients of one
// component and adds its part with a 64-bit vector atomic into the zeroed
// GLWE: exact and order-independent modulo 2^64.
// Grid (N / 256, k + 1, G * N / PK_JC).
constexpr int PK_JC = 32;
__global__ void __launch_bounds__(256) k_pack_rotate(const u64* __restrict__ M, const u64* __restrict__ ct,
                                                     int64_t count, int N, int k, u64* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  const int nch = N / PK_JC;
  const int64_t g = blockIdx.z / nch;
  const int j0 = (int)(blockIdx.z % nch) * PK_JC;
  const int cnt = (int)min((int64_t)N, count - g * N);
  if (j0 >= cnt) return;
  const int jend = min(j0 + PK_JC, cnt);
  const size_t n1 = (size_t)(k + 1) * N;
  u64 acc = 0;
  for (int j = j0; j < jend; ++j) {
    const u64* src = M + (size_t)(g * N + j) * n1 + (size_t)c * N;
    acc += t >= j ? src[t - j] : (u64)0 - src[t - j + N];
  }
  if (c == k && t >= j0 && t < jend) acc += ct[(size_t)(g * N + t) * ((size_t)k * N + 1) + (size_t)k * N];
  atomicAdd((unsigned long long*)&out[((size_t)g * (k + 1) + c) * N + t], (unsigned long long)acc);
}

// Decryption of packed GLWEs, one workgroup each: phase[t] = B[t] - sum_c
// (A_c * S_c)[t] (negacyclic, binary S: exact), decoded as k_decrypt's modes
// (0: signed msg_bits-bit value, 1: bit, 2: raw phase) for the coefficients
// below `count`; out[g * N + t].
__global__ void __launch_bounds__(256) k_decrypt_packed(int N, int k, int msg_bits, int mode,
                                                        const u64* __restrict__ s_big, const u64* __restrict__ glwe,
                                                        int64_t count, int64_t* __restrict__ out) {
  extern __shared__ u64 shm[];
  u64* A = shm;                                  // N
  unsigned char* S = (unsigned char*)(shm + N);  // N
  const int64_t g = blockIdx.x;
  const u64* src = glwe + (size_t)g * (k + 1) * N;
  constexpr int MAXC = 8;
  u64 acc[MAXC];
  const int per = N / 256;
  for (int q = 0; q < per; ++q) acc[q] = 0;
  for (int c = 0; c < k; ++c) {
    for (int t = threadIdx.x; t < N; t += 256) {
      A[t] = src[(size_t)c * N + t];
      S[t] = (unsigned char)s_big[(size_t)c * N + t];
    }
    __syncthreads();
    for (int v = 0; v < N; ++v) {
      if (!S[v]) continue;  // uniform across the block
      for (int q = 0; q < per; ++q) {
        const int t = threadIdx.x + 256 * q;
        acc[q] += (t >= v) ? A[t - v] : (u64)0 - A[t - v + N];
      }
    }
    __syncthreads();
  }
  for (int q = 0; q < per; ++q) {
    const int t = threadIdx.x + 256 * q;
    const int64_t idx = g * N + t;
    if (idx >= count) continue;
    const u64 ph = src[(size_t)k * N + t] - acc[q];
    int64_t r;
    if (mode == 0) {
      u64 v = ((ph >> (63 - msg_bits)) + 1) >> 1;
      if (msg_bits < 64) v &= (1ull << msg_bits) - 1;
      r = (v >> (msg_bits - 1)) ? (int64_t)v - ((int64_t)1 << msg_bits) : (int64_t)v;
    } else if (mode == 1) {
      r = (int64_t)(((ph + (1ull << 62)) >> 63) & 1);
    } else {
      r = (int64_t)ph;
    }
    out[idx] = r;
  }
}
