// The grouped bridge over segments that belong to different tenants of a
// group: every old generation of every participating tenant
// in one digits launch, one GEMM launch and one copy back. Included by
// fheicp.hip after k_bridge_grp.h.
//
// A segment is one non-empty old generation of one tenant: Q_t n_{t,g} compact
// rows, compact row start + q n + j standing for row row0_t + q B_t + doc0 + j
// of the group's padded buffer (row0_t: fhe_group_rows' start of tenant t for
// counts[t] = Q_t B_t). Segments follow each other unpadded in the compact
// buffer, each with ceil(rows / 128) ciphertext blocks and ceil(rows / 16)
// digit groups of its own (KsGrpBlock's convention with "tenant" = segment,
// k_ks_grp_tables builds the block table from starts | ends), so a 128-row
// workgroup never straddles two segments. Up to 64 tenants x 8 generations =
// 512 segments: too many for kernel arguments, so the host writes starts |
// ends | the segment records | the key table in stream order (store_words).
// The GEMM is k_keyswitch_mfma_grp<8, 1> with n1 = kN + 1, R = 0 and the
// segments' byte planes in its key table. Every table read is at a
// workgroup-uniform address (scalar loads). Padding rows, current-key rows and
// the rows of tenants that sit out belong to no segment: they are neither read
// nor written.
#pragma once

#include "common.h"

#define BRIDGE_HUB_SEGS_MAX 512  // 64 tenants x FHE_BRIDGE_SLOTS generations

struct BridgeSeg {
  int64_t start;  // first compact row of the segment
  int64_t n;      // documents of the generation (n_{t,g}); the segment holds Q_t n rows
  int64_t doc0;   // its first document among the tenant's B
  int64_t B;      // the tenant's documents: its result is query-major Q_t x B
  int64_t row0;   // the tenant's first row of the group's padded buffer
};
#define BRIDGE_SEG_WORDS 5  // a record as the host stores it, in u64 words
static_assert(sizeof(BridgeSeg) == 8 * BRIDGE_SEG_WORDS, "BridgeSeg is five words");

// the padded-buffer row of compact row c of segment s (c within the segment)
__device__ __forceinline__ int64_t bridge_seg_row(const BridgeSeg& s, int64_t c) {
  const int64_t r = c - s.start, qi = r / s.n;
  return s.row0 + qi * s.B + s.doc0 + (r - qi * s.n);
}

// k_bridge_digits_grp with the source row through the segment record: grid
// (big / 64, 8 * blocks), 256 threads; block y forms digit group y & 7 of
// ciphertext block y >> 3. Same digits, tie coins and A-fragment layout, the
// body kept (body[c], c the compact row). zero_n1 > 0: the compact output rows
// of the group are zeroed for the split-K atomics. A digit group past the
// segment's rows does not exist: nothing is read or written for it.
__global__ void __launch_bounds__(256) k_bridge_digits_hub(const u64* __restrict__ in,
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
  const int t = threadIdx.x, cl = t >> 4, iq = t & 15;
  const int64_t c = c0 + cl;
  const int i0 = blockIdx.x * 64 + iq * 4;
  if (zero_n1 > 0) {
    const int per = (zero_n1 + (int)gridDim.x - 1) / (int)gridDim.x;
    for (int z = t; z < 16 * per; z += 256) {
      const int q = z / per, col = (int)blockIdx.x * per + (z - q * per);
      const int64_t cz = c0 + q;
      if (cz < e.end && col < zero_n1) zero_out[(size_t)cz * zero_n1 + col] = 0;
    }
  }
  if (c >= e.end) return;
  const u64* src = in + (size_t)bridge_seg_row(sg, c) * (big + 1);
  if (blockIdx.x == 0 && iq == 0) body[c] = src[big];
  const int prec = levels * beta;
  const u64 half = 1ull << (beta - 1), mask = (1ull << beta) - 1;
  uint32_t packed[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) packed[s] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u64 x = src[i0 + q];
    u64 rr = ((x >> (63 - prec)) + 1) >> 1;
#pragma unroll
    for (int s = 0; s < 8; ++s) {  // LSB-first: digit s is level levels - 1 - s
      if (s >= levels) break;
      const u64 low = (rr >> (s * beta)) & mask;
      const u64 coin = (x >> (62 - prec - s)) & 1;
      const int d = (low > half || (low == half && coin)) ? (int)low - (1 << beta) : (int)low;
      rr -= (u64)(int64_t)d << (s * beta);
      packed[s] |= (uint32_t)(uint8_t)(int8_t)d << (8 * q);
    }
  }
  const int lane = cl + 16 * ((i0 >> 4) & 3);
  const int kbi = i0 >> 6, kbl = big >> 6;
  const size_t dg = (size_t)e.dg0 + j;  // the digit group among all segments'
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    const int kb = (levels - 1 - s) * kbl + kbi;
    D[((dg * KB + kb) * 64 + lane) * 4 + ((i0 & 15) >> 2)] = packed[s];
  }
}

// The GEMM's compact rows back to their places in the padded buffer: grid
// (8 * blocks, ceil(n1 / 256)); block x copies the (at most 16) rows of digit
// group x & 7 of ciphertext block x >> 3.
__global__ void __launch_bounds__(256) k_bridge_scatter_hub(const u64* __restrict__ M,
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
