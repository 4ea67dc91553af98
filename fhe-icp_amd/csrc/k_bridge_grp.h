// Group form of the bridge key switch: the rows of several old key generations
// in one digits launch, one GEMM launch and one copy back, each generation
// with its own bridge key. Included by fheicp.hip after
// k_ks_grp.h and k_bridge.h.
//
// Documents are resident oldest generation first: generation g holds the n_g
// documents doc0_g .. doc0_g + n_g - 1 of every query of a query-major Q x B
// result. Its compact segment is Q n_g rows, compact row start_g + q n_g + j
// standing for result row q B + doc0_g + j; the segments follow each other
// unpadded. A segment owns ceil(rows / 128) ciphertext blocks and
// ceil(rows / 16) digit groups of its own (KsGrpBlock's convention with
// "tenant" = generation, k_ks_grp_tables builds the block table from
// starts | ends), so a 128-row workgroup never straddles two generations.
// The GEMM is k_keyswitch_mfma_grp<8, 1> with n1 = kN + 1, R = 0 and the
// generations' byte planes in its key table. Every table read is at a
// workgroup-uniform address (scalar loads).
#pragma once

#include "common.h"

#define BRIDGE_GENS_MAX 8  // = FHE_BRIDGE_SLOTS (include/fhe_icp.h)

struct BridgeGen {
  int64_t start;  // first compact row of the segment
  int64_t n;      // documents of the generation (n_g); the segment holds Q n_g rows
  int64_t doc0;   // its first document
};

// what the host knows of a call, by value: one launch writes every table
struct BridgeGensArg {
  int64_t start[BRIDGE_GENS_MAX], n[BRIDGE_GENS_MAX], doc0[BRIDGE_GENS_MAX];
  const void* planes[BRIDGE_GENS_MAX];
};

// starts | ends (k_ks_grp_tables' input), the generation table and the GEMM's
// key table; one thread per generation
__global__ void k_bridge_grp_setup(BridgeGensArg a, int G, int64_t Q, int64_t* __restrict__ se,
                                   BridgeGen* __restrict__ gen, const void** __restrict__ keys) {
  const int g = threadIdx.x;
  if (g >= G) return;
  se[g] = a.start[g];
  se[G + g] = a.start[g] + Q * a.n[g];
  gen[g] = {a.start[g], a.n[g], a.doc0[g]};
  keys[g] = a.planes[g];
}

// k_bridge_digits over the blocks: grid (big / 64, 8 * blocks), 256 threads;
// block y forms digit group y & 7 of ciphertext block y >> 3. Same digits, tie
// coins and A-fragment layout, the body kept (body[c], c the compact row); the
// source row comes through the block's generation. zero_n1 > 0: the compact
// output rows of the group are zeroed for the split-K atomics. A digit group
// past the segment's rows does not exist: nothing is read or written for it.
__global__ void __launch_bounds__(256) k_bridge_digits_grp(const u64* __restrict__ in,
                                                           const KsGrpBlock* __restrict__ blk,
                                                           const BridgeGen* __restrict__ gen, int64_t B, int big,
                                                           int beta, int levels, int KB, uint32_t* __restrict__ D,
                                                           u64* __restrict__ body, int zero_n1,
                                                           u64* __restrict__ zero_out) {
  const KsGrpBlock e = blk[blockIdx.y >> 3];
  const int j = blockIdx.y & 7;
  const int64_t c0 = e.row0 + (int64_t)j * 16;  // the group's first compact row
  if (c0 >= e.end) return;
  const BridgeGen ge = gen[e.tenant];
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
  const int64_t r = c - ge.start, qi = r / ge.n;
  const u64* src = in + (size_t)(qi * B + ge.doc0 + (r - qi * ge.n)) * (big + 1);
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
  const size_t dg = (size_t)e.dg0 + j;  // the digit group among all generations'
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= levels) break;
    const int kb = (levels - 1 - s) * kbl + kbi;
    D[((dg * KB + kb) * 64 + lane) * 4 + ((i0 & 15) >> 2)] = packed[s];
  }
}

// The GEMM's compact rows back to their places through the same tables: grid
// (8 * blocks, ceil(n1 / 256)); block x copies the (at most 16) rows of digit
// group x & 7 of ciphertext block x >> 3.
__global__ void __launch_bounds__(256) k_bridge_scatter_grp(const u64* __restrict__ M,
                                                            const KsGrpBlock* __restrict__ blk,
                                                            const BridgeGen* __restrict__ gen, int64_t B, int n1,
                                                            u64* __restrict__ out) {
  const KsGrpBlock e = blk[blockIdx.x >> 3];
  const int64_t c0 = e.row0 + (int64_t)(blockIdx.x & 7) * 16;
  if (c0 >= e.end) return;
  const BridgeGen ge = gen[e.tenant];
  const int col = blockIdx.y * 256 + threadIdx.x;
  if (col >= n1) return;
  const int64_t c1 = c0 + 16 < e.end ? c0 + 16 : e.end;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t r = c - ge.start, qi = r / ge.n;
    out[(size_t)(qi * B + ge.doc0 + (r - qi * ge.n)) * n1 + col] = M[(size_t)c * n1 + col];
  }
}
