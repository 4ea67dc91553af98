// Group form of the transposed external product (k_extprod_q.h): the leveled
// step of several key holders in a fixed number of launches.
// Included by fheicp.hip after k_extprod_q.h and k_blind_rotate.h.
//
// Tenant t brings its own Q_t GGSW queries and its own document operand F_t
// (G_t GLWEs); all share (N, k) and the gadget level L, so the K extent
// KB = (k+1) N L / 64 is one for the launch. The query planes of all tenants
// lie in one buffer, tenant t's row tiles (16 rows each, padded to whole groups
// of the launch's RT) from row tile rt0_t on; the results M_t[q][g][c'][t] lie
// in one buffer from word m0_t on; the extracted rows go to the padded group
// layout (fhe_group_rows: tenant t's Q_t B_t rows from start_t, query-major).
// A workgroup finds its work in two tables read at a workgroup-uniform address
// (scalar loads, as BrGrpTenant and KsGrpBlock are): its tile, and through it
// the tenant's record.
#pragma once

// Operands whose pointers come out of a table, in global memory: without the
// address space the compiler emits flat loads for them, which count against
// the LDS counter too (k_ks_grp.h's ksm_gv4i).
typedef __attribute__((address_space(1))) u64 xq_gu64;
typedef __attribute__((address_space(1))) uint8_t xq_gu8;
typedef __attribute__((address_space(1))) v4i_dw xq_gv4dw;
typedef __attribute__((address_space(1))) int xq_gint;

struct XqGrpTenant {
  const u64* ggsw;   // Q GGSWs [Q][c][l][c'][coef]
  const uint8_t* F;  // fhe_glwe_docs_queries_pack of the tenant's B documents
  int64_t start;     // first row of the tenant in the padded layout
  int64_t m0;        // first word of M_t in the result buffer
  int32_t Q, G;
  int32_t B, D;
  int32_t rt0;       // first row tile of the tenant in the plane buffer
  int32_t c0;        // first of the tenant's Q scaled constants
};
// the participating tenants of one call, passed by value to k_xq_grp_tables
// (64 records of 56 bytes: inside the 4 KB of kernel arguments)
constexpr int XQ_GRP_MAX = 64;
struct XqGrpTenants {
  XqGrpTenant v[XQ_GRP_MAX];
};
struct XqGrpTile {
  int32_t tenant;  // index into the records
  int32_t cw;      // column workgroup within the tenant (k_extprod_queries_mfma's blockIdx.x)
  int32_t rg;      // row-tile group within the tenant (its blockIdx.y)
  int32_t pad;
};

__host__ __device__ inline int64_t xq_grp_rtiles(int k, int Q, int RT) {
  const int64_t rtn = ((int64_t)Q * (k + 1) + 15) / 16;
  return (rtn + RT - 1) / RT * RT;
}
__host__ __device__ inline int64_t xq_grp_cgrid(int N, int G) { return (int64_t)G * (N / 16) / XQ_CG; }

// The tables of a call, one thread per entry of the longest: the records
// themselves, tile -> (tenant, column workgroup, row-tile group) with a
// tenant's tiles row group after row group, row tile -> tenant for the planes,
// and row quad -> tenant for the extraction (-1: tenants end before it).
__global__ void __launch_bounds__(256) k_xq_grp_tables(XqGrpTenants h, int nt, int N, int k, int RT, int64_t ntiles,
                                                       int64_t nrt, int64_t nquads, XqGrpTenant* __restrict__ ten,
                                                       XqGrpTile* __restrict__ tiles, int32_t* __restrict__ rt_tenant,
                                                       int32_t* __restrict__ quad_tenant) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nt) ten[i] = h.v[i];
  if (i < ntiles) {
    int64_t t0 = 0;
    for (int u = 0; u < nt; ++u) {
      const int64_t cg = xq_grp_cgrid(N, h.v[u].G), n = cg * (xq_grp_rtiles(k, h.v[u].Q, RT) / RT);
      if (i < t0 + n) {
        const int64_t loc = i - t0;
        tiles[i] = {u, (int32_t)(loc % cg), (int32_t)(loc / cg), 0};
        break;
      }
      t0 += n;
    }
  }
  if (i < nrt) {
    int t = 0;
    for (int u = 0; u < nt; ++u)
      if (h.v[u].rt0 <= i) t = u;
    rt_tenant[i] = t;
  }
  if (i < nquads) {
    int t = -1;  // the tenant whose padded segment holds rows 4 i .. 4 i + 3
    for (int u = 0; u < nt; ++u)
      if (h.v[u].start <= 4 * i) t = u;
    quad_tenant[i] = t;
  }
}

// k_ggsws_planes over the row tiles of all tenants: block (kb, rt) flattened on
// x (rt KB + kb), so no 65,535 bound applies to the row tiles. The tile's
// tenant gives the GGSWs, Q and its first tile; the fragment order within a
// tenant is k_ggsws_planes's.
__global__ void __launch_bounds__(64) k_ggsws_planes_grp(const XqGrpTenant* __restrict__ ten,
                                                         const int32_t* __restrict__ rt_tenant, int N, int k, int L,
                                                         int KB, v4i* __restrict__ out) {
  const int lane = threadIdx.x;
  const int64_t rtg = blockIdx.x / (unsigned)KB;  // row tile of the launch
  const int kb = (int)(blockIdx.x - rtg * KB);
  const XqGrpTenant e = ten[rt_tenant[rtg]];
  const xq_gu64* __restrict__ ggsw = (const xq_gu64*)e.ggsw;
  const int rt = (int)(rtg - e.rt0), kpr = N >> 6;
  const int cl = kb / kpr, s0 = (kb - cl * kpr) * 64 + 16 * (lane >> 4);
  const int rho = rt * 16 + (lane & 15);
  const int q = rho / (k + 1), cp = rho - q * (k + 1);
  uint32_t pk[8][4];
#pragma unroll
  for (int p = 0; p < 8; ++p)
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) pk[p][e4] = 0;
  if (q < e.Q) {
    const xq_gu64* row = ggsw + (((size_t)q * (k + 1) * L + cl) * (k + 1) + cp) * N + s0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      u64 x = row[j];
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int8_t sp = (int8_t)(x & 0xff);
        x = (x - (u64)(int64_t)sp) >> 8;
        pk[p][j >> 2] |= (uint32_t)(uint8_t)sp << (8 * (j & 3));
      }
    }
  }
  v4i* o = out + ((size_t)rtg * KB + kb) * 8 * 64 + lane;
#pragma unroll
  for (int p = 0; p < 8; ++p) o[p * 64] = (v4i){(int)pk[p][0], (int)pk[p][1], (int)pk[p][2], (int)pk[p][3]};
}

// k_extprod_queries_mfma<RT> over the tiles of all tenants: grid (tiles, 1, S),
// tiles flattened on x, so no 65,535 bound applies to row groups or GLWEs. The
// tile's record gives the planes, F, Q, G and M of its tenant; from there on
// the body is k_extprod_queries_mfma's (fragment formation, LDS double buffer,
// epilogue), copied rather than shared, as k_keyswitch_mfma_grp's is: moved
// into a common __device__ function, the single-tenant kernels came out of the
// compiler with other code (docs/AB_LOG_r17.md), and they are what this form
// is tested against. A row rho >= (k+1) Q_t and a block with g >= G_t store
// nothing. One S for the launch: atomics into the zeroed results when S > 1,
// plain stores otherwise.
template <int RT>
__global__ void __launch_bounds__(256, 2) k_extprod_queries_mfma_grp(const XqGrpTile* __restrict__ tiles,
                                                                     const XqGrpTenant* __restrict__ ten,
                                                                     const v4i* __restrict__ P8all, int N, int k,
                                                                     int L, int KB, int kslice,
                                                                     u64* __restrict__ Mall) {
  constexpr int TV = RT * 8 * 64;   // v4i per query tile (one k-block)
  constexpr int TL = TV / 256;      // per thread
  __shared__ v4i at[2][TV];
  const XqGrpTile tl = tiles[blockIdx.x];
  const XqGrpTenant te = ten[tl.tenant];
  const xq_gu8* __restrict__ F = (const xq_gu8*)te.F;
  const int Q = te.Q, G = te.G;
  u64* __restrict__ M = Mall + te.m0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kpr = N >> 6, nbg = N >> 4;  // k-blocks per (c, l) row; column blocks per GLWE
  const int rt0 = tl.rg * RT;
  const int kb_lo = blockIdx.z * kslice, kb_hi = min(KB, kb_lo + kslice);
  const size_t fs = xq_fstride(N);
  const int rowsF = (k + 1) * L;
  // this wave's column blocks
  int g[XQ_CW], t[XQ_CW], sh[XQ_CW];
  const xq_gu8* Fw[XQ_CW];
#pragma unroll
  for (int c = 0; c < XQ_CW; ++c) {
    const int nb = (tl.cw * XQ_WAVES + w) * XQ_CW + c;
    g[c] = nb / nbg;
    const int rem = nb - g[c] * nbg;
#ifdef FHEICP_XQ_STRIDE16
    t[c] = 256 * (rem >> 4) + (rem & 15) + 16 * (lane & 15);
#else
    t[c] = 16 * rem + (lane & 15);
#endif
    const int o = N - 1 - t[c] + 16 * (lane >> 4);  // + s0 (a multiple of 64) per k-block
    sh[c] = o & 3;
    // a block past the tenant's batch streams its GLWE 0's digits and stores nothing
    Fw[c] = F + (size_t)(g[c] < G ? g[c] : 0) * rowsF * fs + (o & ~3);
  }
  const v4i* Pv = P8all + ((size_t)te.rt0 + rt0) * KB * 8 * 64 + tid;
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
      const xq_gu8* p = Fw[c] + (size_t)cl * fs + s0;
      fa[c] = *(const xq_gv4dw*)p;
      fb[c] = *(const xq_gint*)(p + 16);
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

// k_extprod_extract_queries over the padded group rows: row r belongs to the
// tenant of its quad; within the tenant it is document b under query q
// (r - start_t = q B_t + b), from M_t with cst[c0_t + q] (pre-scaled) on the
// body. A padding row is neither read nor written. `cpy`, when given, takes
// the same words: the copy the packings read after the sign extraction has
// consumed `out`. Grid (rows, ceil((kN + 1) / 256)).
__global__ void __launch_bounds__(256) k_extprod_extract_grp(const u64* __restrict__ Mall,
                                                             const XqGrpTenant* __restrict__ ten,
                                                             const int32_t* __restrict__ quad_tenant, int N, int k,
                                                             const u64* __restrict__ cst, u64* __restrict__ out,
                                                             u64* __restrict__ cpy) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  const int64_t r = blockIdx.x;
  const int big = k * N;
  if (col > big) return;
  const int tn = quad_tenant[r >> 2];
  if (tn < 0) return;
  const XqGrpTenant e = ten[tn];
  const int64_t loc = r - e.start;
  if (loc >= (int64_t)e.Q * e.B) return;  // padding row
  const int64_t q = loc / e.B, b = loc - q * e.B;
  const int S = N / e.D;
  const int64_t g = b / S;
  const int p = (int)(b - g * S) * e.D;
  const u64* src = Mall + e.m0 + ((size_t)q * (size_t)e.G + (size_t)g) * (k + 1) * N;
  u64 v;
  if (col == big) {
    v = src[(size_t)k * N + p] + cst[e.c0 + q];
  } else {
    const int c = col / N, u = col - c * N;
    v = u <= p ? src[(size_t)c * N + p - u] : (u64)0 - src[(size_t)c * N + p - u + N];
  }
  const size_t at = (size_t)r * (big + 1) + col;
  out[at] = v;
  if (cpy) cpy[at] = v;
}
