// Both-private search, Q queries in one pass: the external
// product of k_extprod.h transposed, so that nothing of size ((k+1)N)^2 exists.
// With d_{g,c,l} the digit polynomial (k_glwe_digits's digits) of component c
// of document GLWE g at level l and E_{g,c,l}[m] = d[m] for 0 <= m < N,
// -d[m + N] for -N <= m < 0 (negating an int8 digit in [-64, 64] is exact),
//   out[q][g][c'][t] = sum_{p<8} 2^(8p) sum_{c,l} sum_{s<N}
//                        plane_p(Row_q(c,l)[c'][s]) * E_{g,c,l}[t - s]   (mod 2^64),
// a GEMM with rows (q, c'), K = (c, l, s) and columns (g, t). The left operand
// is the GGSWs' own balanced byte planes (k_ggsws_planes); the right operand is
// formed in the GEMM from 2N bytes per (g, c, l) (k_glwe_digits_rev), and the Q
// queries share every document fragment. Part of libfheicp (fheicp.hip
// includes it after k_extprod.h).
#pragma once

#include "common.h"

// Bytes per (g, c, l) of the document operand: F[i] = E[N - 1 - i], i < 2N,
// plus 16 zero bytes the GEMM's five-dword window reads past the end.
__host__ __device__ inline size_t xq_fstride(int N) { return 2 * (size_t)N + 16; }

// The document operand. F is E reversed, so that the 16 k of a fragment lane,
// s = sb + j, read E[t - sb - j] = F[N - 1 - t + sb + j]: 16 ascending bytes.
// The digits are k_glwe_digits's, word for word (same rounding, same coins).
// A thread takes 4 consecutive coefficients m = 4a + q of (g, c) and writes,
// per level, the dword at F[N - 4 - 4a] (d reversed) and the one at
// F[2N - 4 - 4a] (-d reversed). Grid (n1 / 1024, G), 256 threads; the caller
// zeroes the buffer (the 16 tail bytes of every row).
__global__ void __launch_bounds__(256) k_glwe_digits_rev(const u64* __restrict__ in, int N, int k, int beta,
                                                         int levels, uint8_t* __restrict__ F) {
  const int n1 = (k + 1) * N;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n1) return;
  const size_t g = blockIdx.y;
  const int c = i0 / N, m0 = i0 - c * N;
  const u64* src = in + g * n1;
  uint32_t pos[8], neg[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) pos[s] = neg[s] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    glwe_word_digits(src[i0 + q], beta, levels, [&](int s, int d) {
      pos[s] |= (uint32_t)(uint8_t)(int8_t)d << (8 * (3 - q));
      neg[s] |= (uint32_t)(uint8_t)(int8_t)-d << (8 * (3 - q));
    });
  const size_t fs = xq_fstride(N);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    uint8_t* row = F + ((g * (k + 1) + c) * levels + (levels - 1 - s)) * fs;
    *(uint32_t*)(row + (N - 4 - m0)) = pos[s];
    *(uint32_t*)(row + (2 * N - 4 - m0)) = neg[s];
  }
}

// The query operand: the 8 balanced byte planes of Q GGSWs [Q][c][l][c'][coef]
// in A-fragment order [rt][kb][p][lane][16 B]: row tile rt holds rows
// rho = 16 rt + (lane & 15) = q (k+1) + c', k-block kb = (c L + l) N / 64 + s / 64,
// and lane holds s = 64 (kb % (N / 64)) + 16 (lane >> 4) + j in byte j. Rows
// from (k+1) Q up to the padded tile are written as zeros. One thread per
// fragment lane: ggsws_fragment is this lane's part of fragment (rt, kb), o
// the fragment's first plane at this lane. GP: const u64*, or const xq_gu64*
// for GGSWs whose pointer came out of a table (k_extprod_grp.h).
template <typename GP>
__device__ __forceinline__ void ggsws_fragment(GP ggsw, int Q, int rt, int kb, int N, int k, int L, v4i* o) {
  const int lane = threadIdx.x, kpr = N >> 6;
  const int cl = kb / kpr, s0 = (kb - cl * kpr) * 64 + 16 * (lane >> 4);
  const int rho = rt * 16 + (lane & 15);
  const int q = rho / (k + 1), cp = rho - q * (k + 1);
  const GP row = ggsw + (((size_t)q * (k + 1) * L + cl) * (k + 1) + cp) * N + s0;
  byte_planes16_store(q < Q, [&](int j) { return row[j]; }, o);
}
// Grid (KB, RT), 64 threads.
__global__ void __launch_bounds__(64) k_ggsws_planes(const u64* __restrict__ ggsw, int N, int k, int L, int Q,
                                                     v4i* __restrict__ out) {
  const int kb = blockIdx.x, rt = blockIdx.y, KB = gridDim.x;
  ggsws_fragment(ggsw, Q, rt, kb, N, k, L, out + ((size_t)rt * KB + kb) * 8 * 64 + threadIdx.x);
}

// The GEMM. Workgroup = 4 waves = RT row tiles (16 RT rows (q, c')) x 8 column
// blocks x 8 byte planes x one slice of K; each wave owns XQ_CW = 2 column
// blocks, so every query fragment read from LDS feeds two MFMAs.
// Columns: block nb -> g = nb / (N / 16), t = 16 (nb % (N / 16)) + (lane & 15),
// 16 consecutive coefficients. A lane's window of F starts at
// o = N - 1 - t + s0 + 16 (lane >> 4): each lane reads five dwords from the
// dword at o & ~3 (global loads, which take any dword address; the 4 KB of a
// (g, c, l) stay in L1 / L2) and four v_alignbyte_b32 with the lane's own shift
// o & 3 form the fragment. The 64 windows of a wave lie within 83 consecutive
// bytes, one or two cache lines per load, and a block's stores are 128-byte
// runs. Columns 16 apart (-DFHEICP_XQ_STRIDE16) make the shift the same for
// the whole wave but spread a load over 308 bytes: 0.105 against 0.044 ms at
// Q = 8, B = 128 and 0.202 against 0.142 ms at B = 1024 (docs/AB_LOG_r13.md).
// The query tile of a k-block (RT * 8 KB) is shared through two LDS buffers,
// one barrier per k-block: the next tile is loaded into registers before the
// MFMAs and stored into the other buffer after them.
// K is split over gridDim.z workgroups (kslice k-blocks each); partial sums
// are added with 64-bit vector atomics into the zeroed result (exact and
// order-independent modulo 2^64), or stored when there is one slice.
// Result M[q][g][c'][t]. A row rho >= (k+1) Q and a block with g >= G store
// nothing; the q G (k+1) N offset is formed after the guard.
// A/B builds (tools/build_variant.sh): -DFHEICP_XQ_CW=1 (one column block per
// wave), -DFHEICP_XQ_STRIDE16 (above).
#ifndef FHEICP_XQ_CW
#define FHEICP_XQ_CW 2
#endif
constexpr int XQ_CW = FHEICP_XQ_CW, XQ_WAVES = 4, XQ_CG = XQ_CW * XQ_WAVES;  // column blocks per wave / workgroup
typedef int v4i_dw __attribute__((ext_vector_type(4), aligned(4)));
// Operands whose pointers come out of a table (k_extprod_grp.h), in global
// memory: without the address space the compiler emits flat loads for them,
// which count against the LDS counter too (k_ks_grp.h's ksm_gv4i).
typedef __attribute__((address_space(1))) u64 xq_gu64;
typedef __attribute__((address_space(1))) uint8_t xq_gu8;
typedef __attribute__((address_space(1))) v4i_dw xq_gv4dw;
typedef __attribute__((address_space(1))) int xq_gint;
// a lane's five dwords of F, for either kind of pointer
__device__ __forceinline__ v4i_dw xq_ld16(const uint8_t* p) { return *(const v4i_dw*)p; }
__device__ __forceinline__ int xq_ld4(const uint8_t* p) { return *(const int*)p; }
__device__ __forceinline__ v4i_dw xq_ld16(const xq_gu8* p) { return *(const xq_gv4dw*)p; }
__device__ __forceinline__ int xq_ld4(const xq_gu8* p) { return *(const xq_gint*)p; }

// The body of both GEMM kernels, after the prologue in which a kernel finds
// its work (from the grid here, from the tile table in k_extprod_grp.h): the
// LDS double buffer, the fragment formation, the main loop over the k-blocks
// kb_lo .. kb_hi - 1 and the epilogue. Pv: the planes of row tile rt0 at this
// thread; Fw[c] (FP: const uint8_t* or const xq_gu8*), sh[c], g[c], t[c]: the
// window start, byte shift, GLWE and coefficient of this wave's column block c.
template <int RT, typename FP>
__device__ __forceinline__ void xq_gemm_tail(v4i (&at)[2][RT * 8 * 64], const v4i* Pv, const FP (&Fw)[XQ_CW],
                                             const int (&sh)[XQ_CW], const int (&g)[XQ_CW], const int (&t)[XQ_CW],
                                             int rt0, int kb_lo, int kb_hi, int N, int k, int Q, int G, int KB,
                                             u64* __restrict__ M) {
  constexpr int TL = RT * 8 * 64 / 256;  // v4i of a query tile per thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int kpr = N >> 6;  // k-blocks per (c, l) row
  const size_t fs = xq_fstride(N);
  v4i acc[RT][XQ_CW][8];
#pragma unroll
  for (int h = 0; h < RT; ++h)
#pragma unroll
    for (int c = 0; c < XQ_CW; ++c)
#pragma unroll
      for (int p = 0; p < 8; ++p) acc[h][c][p] = (v4i){0, 0, 0, 0};
  v4i ra[TL];
  v4i_dw fa[XQ_CW];
  int fb[XQ_CW];
  // row tile h's fragments of k-block kb are 512 consecutive v4i: two per thread
  auto tile_load = [&](int kb) {
#pragma unroll
    for (int e = 0; e < TL; ++e) ra[e] = Pv[((size_t)(e >> 1) * KB + kb) * 8 * 64 + (e & 1) * 256];
  };
  auto tile_store = [&](v4i* dst) {
#pragma unroll
    for (int e = 0; e < TL; ++e) dst[(e >> 1) * 512 + (e & 1) * 256 + tid] = ra[e];
  };
  auto frag_load = [&](int kb) {
    const int cl = kb / kpr, s0 = (kb - cl * kpr) * 64;
#pragma unroll
    for (int c = 0; c < XQ_CW; ++c) {
      const FP p = Fw[c] + (size_t)cl * fs + s0;
      fa[c] = xq_ld16(p);
      fb[c] = xq_ld4(p + 16);
    }
  };
  tile_load(kb_lo);
  frag_load(kb_lo);
  tile_store(at[0]);
  __syncthreads();
  int cur = 0;
  for (int kb = kb_lo; kb < kb_hi; ++kb) {
    v4i b[XQ_CW];
#pragma unroll
    for (int c = 0; c < XQ_CW; ++c) {
      b[c][0] = (int)__builtin_amdgcn_alignbyte((uint32_t)fa[c][1], (uint32_t)fa[c][0], (uint32_t)sh[c]);
      b[c][1] = (int)__builtin_amdgcn_alignbyte((uint32_t)fa[c][2], (uint32_t)fa[c][1], (uint32_t)sh[c]);
      b[c][2] = (int)__builtin_amdgcn_alignbyte((uint32_t)fa[c][3], (uint32_t)fa[c][2], (uint32_t)sh[c]);
      b[c][3] = (int)__builtin_amdgcn_alignbyte((uint32_t)fb[c], (uint32_t)fa[c][3], (uint32_t)sh[c]);
    }
    const int kn = min(kb + 1, kb_hi - 1);  // clamped: the last step reloads its own
    tile_load(kn);
    frag_load(kn);
#pragma unroll
    for (int h = 0; h < RT; ++h)
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const v4i a = at[cur][(h * 8 + p) * 64 + lane];
#pragma unroll
        for (int c = 0; c < XQ_CW; ++c)
          acc[h][c][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[c], acc[h][c][p], 0, 0, 0);
      }
    tile_store(at[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }
  const int rows = (k + 1) * Q;
  const bool split = gridDim.z > 1;
#pragma unroll
  for (int c = 0; c < XQ_CW; ++c) {
    if (g[c] >= G) continue;
#pragma unroll
    for (int h = 0; h < RT; ++h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rho = (rt0 + h) * 16 + 4 * (lane >> 4) + r;
        if (rho >= rows) continue;
        const int q = rho / (k + 1), cp = rho - q * (k + 1);
        u64 lo = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) lo += (u64)((int64_t)acc[h][c][p][r] * (int64_t)(1 << (8 * p)));
        uint32_t hi = 0;
#pragma unroll
        for (int p = 4; p < 8; ++p) hi += (uint32_t)acc[h][c][p][r] << (8 * (p - 4));
        const u64 v = lo + ((u64)hi << 32);
        u64* dst = M + (((size_t)q * G + g[c]) * (k + 1) + cp) * N + t[c];
        if (split)
          atomicAdd((unsigned long long*)dst, (unsigned long long)v);
        else
          *dst = v;
      }
    }
  }
}

template <int RT>
__global__ void __launch_bounds__(256, 2) k_extprod_queries_mfma(const v4i* __restrict__ P8,
                                                                 const uint8_t* __restrict__ F, int N, int k, int L,
                                                                 int Q, int G, int KB, int kslice,
                                                                 u64* __restrict__ M) {
  __shared__ v4i at[2][RT * 8 * 64];  // two query tiles (one k-block each)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nbg = N >> 4;  // column blocks per GLWE
  const int rt0 = blockIdx.y * RT;
  const int kb_lo = blockIdx.z * kslice, kb_hi = min(KB, kb_lo + kslice);
  const size_t fs = xq_fstride(N);
  const int rowsF = (k + 1) * L;
  // this wave's column blocks
  int g[XQ_CW], t[XQ_CW], sh[XQ_CW];
  const uint8_t* Fw[XQ_CW];
#pragma unroll
  for (int c = 0; c < XQ_CW; ++c) {
    const int nb = (blockIdx.x * XQ_WAVES + w) * XQ_CW + c;
    g[c] = nb / nbg;
    const int rem = nb - g[c] * nbg;
#ifdef FHEICP_XQ_STRIDE16
    t[c] = 256 * (rem >> 4) + (rem & 15) + 16 * (lane & 15);
#else
    t[c] = 16 * rem + (lane & 15);
#endif
    const int o = N - 1 - t[c] + 16 * (lane >> 4);  // + s0 (a multiple of 64) per k-block
    sh[c] = o & 3;
    // a block past the batch streams GLWE 0's digits and stores nothing
    Fw[c] = F + (size_t)(g[c] < G ? g[c] : 0) * rowsF * fs + (o & ~3);
  }
  const v4i* Pv = P8 + (size_t)rt0 * KB * 8 * 64 + tid;
  xq_gemm_tail<RT>(at, Pv, Fw, sh, g, t, rt0, kb_lo, kb_hi, N, k, Q, G, KB, M);
}

// k_extprod_extract with the query on the grid: row q B + b of out is document
// b under query q (M + q G (k+1) N), with cst[q] (device, pre-scaled) on the
// body. Grid (B, ceil((kN + 1) / 256), Q).
__global__ void __launch_bounds__(256) k_extprod_extract_queries(const u64* __restrict__ M, int S, int D, int N, int k,
                                                                 int64_t G, int64_t B, const u64* __restrict__ cst,
                                                                 u64* __restrict__ out) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  const int64_t b = blockIdx.x;
  const size_t q = blockIdx.z;
  const int big = k * N;
  if (col > big) return;
  const int64_t g = b / S;
  const int p = (int)(b - g * S) * D;
  const u64* src = M + (q * (size_t)G + (size_t)g) * (k + 1) * N;
  out[(q * (size_t)B + (size_t)b) * (big + 1) + col] = xq_extract_word(src, p, col, N, k, cst[q]);
}
