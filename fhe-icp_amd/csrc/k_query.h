// Private-query search: one encrypted query against a clear document store.
// Part of libfheicp (one translation unit: fheicp.hip includes it after
// k_server.h, whose v4i and fragment layouts it shares).
//
//   out[b] = sum_j dq[b][j] * (w[j] * ct_q[j]) + trivial(cst * Delta)
//
// for D query ciphertexts ct_q (D x W words, W = kN + 1) and B clear
// documents dq (i8), an integer GEMM [B x D] . [D x W] over Z_2^64. The
// weighted query words are split into 8 balanced radix-256 byte planes,
// x = sum_q s_q 2^(8q) with s_q in [-128, 127] (the last carry dropped: it is
// a multiple of 2^64), each plane an i8 GEMM with i32 accumulation
// (|sum| <= D * 2^14, D <= 65536), recombined as sum_q acc_q << 8q modulo 2^64
// in the epilogue: bit-identical to the plain u64 sum.
// Several queries of one key holder share the documents in one launch, the
// query a grid dimension of the plane and GEMM kernels.
#pragma once

#include "common.h"

// documents (int64 in [-128, 127], B x D row-major) -> A-fragments
// [cb][kb][lane][16 B] as k_ks_digits writes them: lane l of (cb, kb) holds
// document 16 cb + (l & 15), features 64 kb + 16 (l >> 4) + j in byte j; zero
// past B and past D. One thread per fragment lane (a 128-byte read, a 16-byte
// write). Runs once per resident corpus.
__global__ void __launch_bounds__(256) k_query_docs_pack(const int64_t* __restrict__ dq, int64_t B, int D, int KB,
                                                         int64_t ncb, v4i* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= ncb * KB * 64) return;
  const int lane = (int)(e & 63);
  const int64_t f = e >> 6, cb = f / KB;
  const int kb = (int)(f - cb * KB);
  const int64_t doc = cb * 16 + (lane & 15);
  const int k0 = kb * 64 + 16 * (lane >> 4);
  uint32_t pk[4] = {0, 0, 0, 0};
  if (doc < B) {
    const int64_t* src = dq + (size_t)doc * D + k0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (k0 + j < D) pk[j >> 2] |= (uint32_t)(uint8_t)(int8_t)src[j] << (8 * (j & 3));
  }
  out[e] = (v4i){(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
}

// query planes in B-fragment order [kb][nb][q][lane][16 B], q < 8 (as
// k_ksk_to_i8): lane l of (kb, nb) holds column 16 nb + (l & 15), rows
// 64 kb + 16 (l >> 4) + j in byte j, of plane q of w[row] * ct[row][col]
// (mod 2^64: any 64-bit weight; the encoding rescale folds in here). Rows
// past D and columns past W are zero. One wave (= workgroup) per fragment,
// one thread per fragment lane: 16 words in, eight 16-byte stores out (the
// wave writes 1 KB runs). The loads are unconditional (rows clamped to D - 1,
// their weight zeroed), so a lane has all 16 in flight at once; at D = 16 the
// grid is 129 waves, spread over as many CUs. A batch of queries
// (ct [Q][D][W]) puts the query on grid y: the same layout once per query,
// [q][kb][nb][plane][lane].
__global__ void __launch_bounds__(64) k_query_planes(const u64* __restrict__ ct, int D, int W, int NB, int KB,
                                                     const int64_t* __restrict__ w, v4i* __restrict__ out) {
  const int lane = threadIdx.x, f = blockIdx.x;  // grid = KB * NB x Q
  ct += (size_t)blockIdx.y * D * W;
  out += (size_t)blockIdx.y * KB * NB * 8 * 64;
  const int kb = f / NB, nb = f - kb * NB;
  const int col = nb * 16 + (lane & 15);
  const int r0 = kb * 64 + 16 * (lane >> 4);
  const bool live = col < W && r0 < D;
  u64 xs[16];
  if (live) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = min(r0 + j, D - 1);
      xs[j] = ct[(size_t)r * W + col] * (r0 + j < D ? (u64)w[r] : (u64)0);
    }
  }
  byte_planes16_store(live, [&](int j) { return xs[j]; }, out + ((size_t)kb * NB + nb) * 8 * 64 + lane);
}

// The GEMM. A wave owns LQ_RB 16-document groups x LQ_CB 16-column blocks x
// the 8 planes (LQ_RB * LQ_CB * 32 accumulator registers): a plane fragment
// feeds LQ_RB MFMAs and a document fragment LQ_CB * 8. A workgroup is 4 waves
// on consecutive document groups of one column group (their plane fragments
// are the same lines, served by the L1/L2). 2 x 1 measured fastest of 2 x 2,
// 1 x 2, 1 x 4, 4 x 1, 2 x 4 and 4 x 2 at B = 1024 (docs/AB_LOG_r07.md).
// K = D is short (one k-block at D = 16, twelve at 768), so it is not split
// and there are no atomics; at D = 16 the kernel is bound by its stores. In
// the C layout (row 4 (l >> 4) + reg, column l & 15) the 16 lanes of a row
// write 16 consecutive u64: one 128-byte run per row and store instruction.
// Only the real B rows and W columns are stored; groups past the batch or
// the last column block read clamped fragments and store nothing.
#ifndef FHEICP_LQ_RB
#define FHEICP_LQ_RB 2  // A/B builds (tools/build_variant.sh): other wave tiles
#endif
#ifndef FHEICP_LQ_CB
#define FHEICP_LQ_CB 1
#endif
constexpr int LQ_RB = FHEICP_LQ_RB, LQ_CB = FHEICP_LQ_CB;
// KBC: the k-block count as a compile-time constant (0: KB at run time)
template <int KBC = 0>
__device__ __forceinline__ void lq_wave_tile(const v4i* __restrict__ A, const v4i* __restrict__ P8, int64_t B, int W,
                                             int NB, int KB, u64 cst_scaled, u64* __restrict__ out) {
  if (KBC) KB = KBC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ncb = (B + 15) / 16;
  const int64_t rg0 = ((int64_t)blockIdx.x * 4 + wv) * LQ_RB;
  const int cb0 = blockIdx.y * LQ_CB;
  if (rg0 >= ncb) return;  // no barriers below: a whole wave may leave
  const v4i* Av[LQ_RB];
  const v4i* Pv[LQ_CB];
#pragma unroll
  for (int h = 0; h < LQ_RB; ++h) Av[h] = A + (size_t)(rg0 + h < ncb ? rg0 + h : rg0) * KB * 64 + lane;
#pragma unroll
  for (int c = 0; c < LQ_CB; ++c) Pv[c] = P8 + (size_t)min(cb0 + c, NB - 1) * 8 * 64 + lane;
  v4i acc[LQ_RB][LQ_CB][8];
#pragma unroll
  for (int h = 0; h < LQ_RB; ++h)
#pragma unroll
    for (int c = 0; c < LQ_CB; ++c)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[h][c][q] = (v4i){0, 0, 0, 0};
  for (int kb = 0; kb < KB; ++kb) {
    v4i a[LQ_RB];
#pragma unroll
    for (int h = 0; h < LQ_RB; ++h) a[h] = Av[h][(size_t)kb * 64];
#pragma unroll
    for (int c = 0; c < LQ_CB; ++c)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const v4i bq = Pv[c][((size_t)kb * NB * 8 + q) * 64];
#pragma unroll
        for (int h = 0; h < LQ_RB; ++h)
          acc[h][c][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[h], bq, acc[h][c][q], 0, 0, 0);
      }
  }
#pragma unroll
  for (int c = 0; c < LQ_CB; ++c) {
    const int col = (cb0 + c) * 16 + (lane & 15);
    if (cb0 + c >= NB || col >= W) continue;
#pragma unroll
    for (int h = 0; h < LQ_RB; ++h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = (rg0 + h) * 16 + 4 * (lane >> 4) + r;
        if (row >= B) continue;
        // sum_q (int64)acc_q << 8q mod 2^64: planes 0-3 as 64-bit
        // multiply-adds by 2^(8q); planes 4-7 reach only the high word, so
        // they combine in 32 bits
        u64 lo = col == W - 1 ? cst_scaled : (u64)0;
#pragma unroll
        for (int q = 0; q < 4; ++q) lo += (u64)((int64_t)acc[h][c][q][r] * (int64_t)(1 << (8 * q)));
        uint32_t hi = 0;
#pragma unroll
        for (int q = 4; q < 8; ++q) hi += (uint32_t)acc[h][c][q][r] << (8 * (q - 4));
        out[(size_t)row * W + col] = lo + ((u64)hi << 32);
      }
    }
  }
}

__global__ void __launch_bounds__(256, 2) k_linear_query_mfma(const v4i* __restrict__ A, const v4i* __restrict__ P8,
                                                           int64_t B, int W, int NB, int KB, u64 cst_scaled,
                                                           u64* __restrict__ out) {
  lq_wave_tile(A, P8, B, W, NB, KB, cst_scaled, out);
}

// Q queries against the same documents, the query on grid z: query q reads
// its own planes (P8 + q KB NB 8 fragments) and constant (cst_scaled[q], a
// device array) and owns output rows [q B, (q + 1) B). The document fragments
// are the same lines for every q. B need not be a multiple of 16, so a
// query's rows do not start on a 16-row boundary: the row guard stays
// `row < B` inside the query (lq_wave_tile), the q B offset is added after it,
// and a wave's padded rows never reach the next query's.
// -DFHEICP_LQ_QLOOP (A/B builds) launches grid z = 1 instead and lets each
// wave loop over the Q queries, its document fragments loop-invariant (in
// registers at one k-block, from the L1 beyond). Measured slower at every
// shape tried: Q = 8, B = 128: 23.0 against 17.5 us at D = 16 (it leaves 129
// workgroups for 256 CUs), 154.1 against 73.4 us at D = 768
// (docs/AB_LOG_r11.md).
__global__ void __launch_bounds__(256, 2) k_linear_queries_mfma(const v4i* __restrict__ A, const v4i* __restrict__ P8,
                                                             int64_t B, int W, int NB, int KB,
                                                             const u64* __restrict__ cst_scaled,
                                                             u64* __restrict__ out, int Q) {
#ifdef FHEICP_LQ_QLOOP
  for (size_t q = 0; q < (size_t)Q; ++q) {
    if (KB == 1)
      lq_wave_tile<1>(A, P8 + q * NB * 8 * 64, B, W, NB, 1, cst_scaled[q], out + q * (size_t)B * W);
    else
      lq_wave_tile(A, P8 + q * KB * NB * 8 * 64, B, W, NB, KB, cst_scaled[q], out + q * (size_t)B * W);
  }
#else
  const size_t q = blockIdx.z;
  (void)Q;
  lq_wave_tile(A, P8 + q * KB * NB * 8 * 64, B, W, NB, KB, cst_scaled[q], out + q * (size_t)B * W);
#endif
}

// one device word (the stream id of a seeded query for k_expand_seeded)
__global__ void k_store_word(u64* __restrict__ p, u64 v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *p = v;
}

// up to 32 device words from the kernel's arguments (a batch of queries'
// pre-scaled constants and thresholds): no host buffer outlives the call
struct Words32 {
  u64 v[32];
};
__global__ void k_store_words(u64* __restrict__ p, int n, Words32 w) {
  if (blockIdx.x == 0 && (int)threadIdx.x < n) p[threadIdx.x] = w.v[threadIdx.x];
}

// out[i] = v[i] + T[i / B]: query i / B's threshold back onto its B results
__global__ void k_add_query_scalar(const int64_t* __restrict__ v, int64_t n, int64_t B, const int64_t* __restrict__ T,
                                   int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v[i] + T[i / B];
}
