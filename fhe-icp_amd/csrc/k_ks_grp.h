// Group form of the i8 MFMA key switch: one digits launch and one GEMM launch
// over several key holders. Included by fheicp.hip after
// k_server.h.
//
// Rows are §8.11's padded layout (tenant t: n_t real rows at start_t, M rows
// in all). Tenant t owns ceil(n_t / 16) digit groups and ceil(n_t / 128)
// ciphertext blocks of its own, numbered tenant after tenant, so a
// 128-ciphertext workgroup never straddles two tenants and the padding rows
// start_t + n_t .. start_{t+1} - 1 are neither read nor written. A block's
// table entry gives its tenant, its first padded row, its first digit group
// and the tenant's end row; the tenant's key planes come from the group's
// key-pointer table. Every table read is at a workgroup-uniform address
// (scalar loads), so the state lives in scalar registers, as BrGrpTenant does.
#pragma once

typedef __attribute__((address_space(1))) v4i ksm_gv4i;  // a v4i in global memory

struct KsGrpBlock {
  int32_t tenant;
  int32_t dg0;   // first digit group of the block (8 per block; a tenant's last block may own fewer)
  int64_t row0;  // first padded row of the block: start_t + 128 * (block within the tenant)
  int64_t end;   // start_t + n_t
};

// se = starts | ends (k_grp_tables' input); one thread per ciphertext block
__global__ void k_ks_grp_tables(const int64_t* __restrict__ se, int T, int64_t nblk, KsGrpBlock* __restrict__ blk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nblk) return;
  int64_t b0 = 0, dg = 0;
  for (int u = 0; u < T; ++u) {
    const int64_t n = se[T + u] - se[u], nb = (n + KSM_CTS - 1) / KSM_CTS;
    if (i < b0 + nb) {
      const int64_t loc = i - b0;
      blk[i] = {u, (int32_t)(dg + loc * (KSM_CTS / 16)), se[u] + loc * KSM_CTS, se[T + u]};
      return;
    }
    b0 += nb;
    dg += (n + 15) / 16;
  }
}

// k_ks_digits over the blocks: grid (big / 64, 8 * blocks), 256 threads; block
// y forms digit group y & 7 of ciphertext block y >> 3 from its tenant's rows
// (in, body and zero_out are the whole M-row buffers, D the digit groups of
// all tenants). A digit group past the tenant's rows does not exist: nothing
// is read or written for it.
__global__ void __launch_bounds__(256) k_ks_digits_grp(const u64* __restrict__ in,
                                                       const KsGrpBlock* __restrict__ blk, int big, int beta,
                                                       int levels, int shift, u64 add_body, int KB,
                                                       uint32_t* __restrict__ D, u64* __restrict__ body, int zero_n1,
                                                       u64* __restrict__ zero_out) {
  const KsGrpBlock e = blk[blockIdx.y >> 3];
  const int j = blockIdx.y & 7;
  const int64_t left = e.end - e.row0, count = left < KSM_CTS ? left : KSM_CTS;  // the block's real rows
  if ((int64_t)j * 16 >= count) return;
  ks_digits_group(in + (size_t)e.row0 * (big + 1), count, big, beta, levels, shift, add_body, KB,
                  D + (size_t)e.dg0 * KB * 256, body + e.row0, zero_n1, zero_out + (size_t)e.row0 * zero_n1, j);
}

// k_keyswitch_mfma over the blocks: grid (blocks x column groups x S); the
// logical index splits as there, its ciphertext block indexes the table, and
// the digits, key planes, body, row count and output rows are the entry's.
// keys[t] is tenant t's ksk8. From the table read on, the body is
// k_keyswitch_mfma's (ring, LDS tile passing, epilogue), copied rather than
// shared: sharing it through a __device__ function changed the single-key
// kernels' registers and code (docs/AB_LOG_r16.md).
template <int QP, int CB>
__global__ void __launch_bounds__(256, 2) k_keyswitch_mfma_grp(const v4i* __restrict__ Dall,
                                                            const v4i* const* __restrict__ keys,
                                                            const KsGrpBlock* __restrict__ blk,
                                                            const u64* __restrict__ body_all, int n1, int NB, int KB,
                                                            int R, int S, int kslice, u64* __restrict__ out_all) {
  constexpr int KP = FHEICP_KS_KP;
  constexpr int TV = CB * QP * 64;          // v4i per key tile (one k-block, CB column blocks)
  constexpr int TL = (TV + 255) / 256;      // tile words per thread
  __shared__ v4i bt[3][KP][TV];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // k_keyswitch_mfma's XCD-aware order over the (column group, ciphertext
  // block, K slice) grid; the ciphertext block indexes the table
  const int nblk = (int)gridDim.x, bid = (int)blockIdx.x, xcd = bid & 7, q8 = nblk >> 3, r8 = nblk & 7;
  const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int NG = NB / CB;                   // column groups (NB padded to a multiple of CB)
  const int per = nblk / NG;                // ciphertext blocks x slices per column group
  const int ng = t / per, rest = t - ng * per, gb = rest / S, sl = rest - gb * S;
  // the block's tenant: its digit groups, key planes, bodies, real rows and
  // output rows (workgroup-uniform: scalar registers)
  const KsGrpBlock be = blk[gb];
  const int64_t left = be.end - be.row0, count = left < KSM_CTS ? left : KSM_CTS;
  const v4i* __restrict__ D = Dall + (size_t)be.dg0 * KB * 64;
  // the key pointer comes out of memory: without the global address space
  // the compiler emits flat loads for the key tiles, which count against
  // lgkmcnt too and serialise the ring behind the LDS reads
  const ksm_gv4i* __restrict__ K8 = (const ksm_gv4i*)keys[be.tenant];
  const u64* __restrict__ body = body_all + be.row0;
  u64* __restrict__ out = out_all + (size_t)be.row0 * n1;
  constexpr int ctb = 0;                    // the block is its own batch of at most 128 ciphertexts
  const int kb_lo = sl * kslice, kb_hi = min(KB, kb_lo + kslice);
  const int64_t ncb = (count + 15) / 16;   // 16-ciphertext groups (digit rows)
  const int64_t cb0 = (int64_t)ctb * (KSM_CTS / 16) + 2 * w;
  // a group past the batch streams group 0's digits and stores nothing
  const v4i* Dv0 = D + (size_t)(cb0 < ncb ? cb0 : 0) * KB * 64 + lane;
  const v4i* Dv1 = D + (size_t)(cb0 + 1 < ncb ? cb0 + 1 : 0) * KB * 64 + lane;
  const ksm_gv4i* Kv = K8 + (size_t)ng * TV;
  const size_t kstride = (size_t)NB * QP * 64;  // v4i per k-block of the key
  v4i acc[2][CB][QP];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int q = 0; q < QP; ++q) acc[h][c][q] = (v4i){0, 0, 0, 0};
  v4i rk[KSM_RING][TL], rd[KSM_RING][2];
  auto tile_load = [&](v4i(&r)[TL], int kb) {
#pragma unroll
    for (int e = 0; e < TL; ++e)
      if (e * 256 + tid < TV) r[e] = Kv[kb * kstride + e * 256 + tid];
  };
  auto tile_store = [&](v4i* dst, const v4i(&r)[TL]) {
#pragma unroll
    for (int e = 0; e < TL; ++e)
      if (e * 256 + tid < TV) dst[e * 256 + tid] = r[e];
  };
  // prologue: k-blocks lo..lo+3 in flight, the first step's tiles into LDS
#pragma unroll
  for (int j = 0; j < KSM_RING; ++j) {
    tile_load(rk[j], kb_lo + j);
    rd[j][0] = Dv0[(size_t)(kb_lo + j) * 64];
    rd[j][1] = Dv1[(size_t)(kb_lo + j) * 64];
  }
#pragma unroll
  for (int h = 0; h < KP; ++h) tile_store(bt[0][h], rk[h]);
  // steps of KP k-blocks, one barrier each; the ring slots of a step's
  // k-blocks (in LDS since the previous step) reload k-block k + 4, and the
  // next step's tiles (loaded one or two steps ago) go into its LDS buffer
  for (int kb = kb_lo; kb < kb_hi; kb += KSM_RING) {
#pragma unroll
    for (int j0 = 0; j0 < KSM_RING; j0 += KP) {
      const int k0 = kb + j0, step = (k0 - kb_lo) / KP;
#pragma unroll
      for (int h = 0; h < KP; ++h) tile_load(rk[j0 + h], min(k0 + h + KSM_RING, kb_hi - 1));  // clamped: reloads
      if (k0 + KP < kb_hi) {
#pragma unroll
        for (int h = 0; h < KP; ++h) tile_store(bt[(step + 1) % 3][h], rk[(j0 + KP + h) % KSM_RING]);
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < KP; ++h) {
        const v4i a0 = rd[j0 + h][0], a1 = rd[j0 + h][1];
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
          for (int q = 0; q < QP; ++q) {
            const v4i bq = bt[step % 3][h][(c * QP + q) * 64 + lane];
            acc[0][c][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bq, acc[0][c][q], 0, 0, 0);
            acc[1][c][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bq, acc[1][c][q], 0, 0, 0);
          }
        const int kn = min(k0 + h + KSM_RING, kb_hi - 1);
        rd[j0 + h][0] = Dv0[(size_t)kn * 64];
        rd[j0 + h][1] = Dv1[(size_t)kn * 64];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    const int col = (ng * CB + c) * KSM_NB_COLS + (lane & 15);
    if (col >= n1) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (cb0 + h >= ncb) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ci = (cb0 + h) * 16 + 4 * (lane >> 4) + r;
        if (ci >= count) continue;
        u64 v = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) v += (u64)(int64_t)acc[h][c][q][r] << (R + 8 * q);
        const u64 o = (col == n1 - 1 && sl == 0 ? body[ci] : (u64)0) - v;
        if (S == 1)
          out[(size_t)ci * n1 + col] = o;
        else
          atomicAdd((unsigned long long*)&out[(size_t)ci * n1 + col], (unsigned long long)o);
      }
    }
  }
}
