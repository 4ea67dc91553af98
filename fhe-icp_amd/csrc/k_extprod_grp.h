// Segmented form of the transposed external product (k_extprod_q.h): the
// leveled step of several key holders, or of several key
// generations of one holder (§8.19), in a fixed number of launches. Included
// by fheicp.hip after k_extprod_q.h and k_blind_rotate.h.
//
// Segment t (a tenant, or a generation with documents) brings its own Q_t GGSW
// queries and its own document operand F_t (G_t GLWEs); all share (N, k) and
// the gadget level L, so the K extent KB = (k+1) N L / 64 is one for the
// launch. The query planes of all segments lie in one buffer, segment t's row
// tiles (16 rows each, padded to whole groups of the launch's RT) from row
// tile rt0_t on; the results M_t[q][g][c'][t] lie in one buffer from word m0_t
// on. A workgroup finds its work in two tables read at a workgroup-uniform
// address (scalar loads, as BrGrpTenant and KsGrpBlock are): its tile, and
// through it the segment's record. The tables, the planes and the GEMM are one
// for both forms; the extraction differs in where a row goes:
//   tenants      the padded group layout (fhe_group_rows: tenant t's Q_t B_t
//                rows from start_t, query-major), k_extprod_extract_grp;
//   generations  ONE query-major Q x B matrix (row q B + off_g + b, off_g the
//                documents before generation g), the layout the segmented
//                bridge (k_bridge.h) takes its row map over,
//                k_extprod_extract_gens. Every generation has the same Q and D.
#pragma once

struct XqGrpTenant {
  const u64* ggsw;   // Q GGSWs [Q][c][l][c'][coef]
  const uint8_t* F;  // fhe_glwe_docs_queries_pack of the segment's B documents
  int64_t start;     // first row of the tenant in the padded layout; off_g of a generation
  int64_t m0;        // first word of M_t in the result buffer
  int32_t Q, G;
  int32_t B, D;
  int32_t rt0;       // first row tile of the segment in the plane buffer
  int32_t c0;        // first of the segment's Q scaled constants
};
// The segments of one call, passed by value to k_xq_tables<CAP>: 64 records of
// 56 bytes are inside the 4 KB of kernel arguments; a call of up to
// XQ_GENS_MAX segments passes that many (0.5 KB: the 3.5 KB cost the
// generations' leveled step 0.013 ms of 0.061, docs/AB_LOG_r24.md).
constexpr int XQ_GRP_MAX = 64;
constexpr int XQ_GENS_MAX = FHE_BRIDGE_SLOTS + 1;  // every bridge slot's generation and the current one
static_assert(XQ_GENS_MAX <= XQ_GRP_MAX, "the generations of a call are segments of one table");
template <int CAP>
struct XqSegs {
  XqGrpTenant v[CAP];
};
struct XqGrpTile {
  int32_t tenant;  // index into the records
  int32_t cw;      // column workgroup within the segment (k_extprod_queries_mfma's blockIdx.x)
  int32_t rg;      // row-tile group within the segment (its blockIdx.y)
  int32_t pad;
};

__host__ __device__ inline int64_t xq_grp_rtiles(int k, int Q, int RT) {
  const int64_t rtn = ((int64_t)Q * (k + 1) + 15) / 16;
  return (rtn + RT - 1) / RT * RT;
}
__host__ __device__ inline int64_t xq_grp_cgrid(int N, int G) { return (int64_t)G * (N / 16) / XQ_CG; }

// The tables of a call, one thread per entry of the longest: the records
// themselves, tile -> (segment, column workgroup, row-tile group) with a
// segment's tiles row group after row group, row tile -> segment for the
// planes, and what the form's extraction finds a row's segment by: row quad ->
// tenant (-1: tenants end before it) when nquads > 0, the segments' document
// ends when `ends` is given.
template <int CAP>
__global__ void __launch_bounds__(256) k_xq_tables(XqSegs<CAP> h, int nt, int N, int k, int RT, int64_t ntiles,
                                                   int64_t nrt, int64_t nquads, XqGrpTenant* __restrict__ ten,
                                                   XqGrpTile* __restrict__ tiles, int32_t* __restrict__ rt_tenant,
                                                   int32_t* __restrict__ quad_tenant, int64_t* __restrict__ ends) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nt) {
    ten[i] = h.v[i];
    if (ends) ends[i] = h.v[i].start + h.v[i].B;
  }
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

// k_ggsws_planes over the row tiles of all segments: block (kb, rt) flattened on
// x (rt KB + kb), so no 65,535 bound applies to the row tiles. The tile's
// segment gives the GGSWs, Q and its first tile; the fragment within a segment
// is k_ggsws_planes's (ggsws_fragment).
__global__ void __launch_bounds__(64) k_ggsws_planes_grp(const XqGrpTenant* __restrict__ ten,
                                                         const int32_t* __restrict__ rt_tenant, int N, int k, int L,
                                                         int KB, v4i* __restrict__ out) {
  const int64_t rtg = blockIdx.x / (unsigned)KB;  // row tile of the launch
  const int kb = (int)(blockIdx.x - rtg * KB);
  const XqGrpTenant e = ten[rt_tenant[rtg]];
  ggsws_fragment((const xq_gu64*)e.ggsw, e.Q, (int)(rtg - e.rt0), kb, N, k, L,
                 out + ((size_t)rtg * KB + kb) * 8 * 64 + threadIdx.x);
}

// k_extprod_queries_mfma<RT> over the tiles of all segments: grid (tiles, 1, S),
// tiles flattened on x, so no 65,535 bound applies to row groups or GLWEs. The
// tile's record gives the planes, F, Q, G and M of its segment; from there on
// the body is k_extprod_queries_mfma's (xq_gemm_tail). A row rho >= (k+1) Q_t
// and a block with g >= G_t store nothing. One S for the launch: atomics into
// the zeroed results when S > 1, plain stores otherwise.
template <int RT>
__global__ void __launch_bounds__(256, 2) k_extprod_queries_mfma_grp(const XqGrpTile* __restrict__ tiles,
                                                                     const XqGrpTenant* __restrict__ ten,
                                                                     const v4i* __restrict__ P8all, int N, int k,
                                                                     int L, int KB, int kslice,
                                                                     u64* __restrict__ Mall) {
  __shared__ v4i at[2][RT * 8 * 64];  // two query tiles (one k-block each)
  const XqGrpTile tl = tiles[blockIdx.x];
  const XqGrpTenant te = ten[tl.tenant];
  const xq_gu8* __restrict__ F = (const xq_gu8*)te.F;
  const int Q = te.Q, G = te.G;
  u64* __restrict__ M = Mall + te.m0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nbg = N >> 4;  // column blocks per GLWE
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
    // a block past the segment's batch streams its GLWE 0's digits and stores nothing
    Fw[c] = F + (size_t)(g[c] < G ? g[c] : 0) * rowsF * fs + (o & ~3);
  }
  const v4i* Pv = P8all + ((size_t)te.rt0 + rt0) * KB * 8 * 64 + tid;
  xq_gemm_tail<RT>(at, Pv, Fw, sh, g, t, rt0, kb_lo, kb_hi, N, k, Q, G, KB, M);
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
  const u64 v = xq_extract_word(src, p, col, N, k, cst[e.c0 + q]);
  const size_t at = (size_t)r * (big + 1) + col;
  out[at] = v;
  if (cpy) cpy[at] = v;
}

// k_extprod_extract_queries over the Q x B rows of all generations: row
// r = q B + x is document x of the call under query q. Its segment is the
// first whose end lies beyond x (the ends table, read at a workgroup-uniform
// address: a workgroup is one row); within the segment it is document
// b = x - off_g, read from M_g with k_extprod_extract_grp's index arithmetic,
// cst[q] (pre-scaled) on the body. Grid (Q B, ceil((kN + 1) / 256)): no row
// beyond Q B exists, a thread per word of the row, consecutive threads
// consecutive words.
__global__ void __launch_bounds__(256) k_extprod_extract_gens(const u64* __restrict__ Mall,
                                                              const XqGrpTenant* __restrict__ ten,
                                                              const int64_t* __restrict__ ends, int ns, int64_t B,
                                                              int N, int k, const u64* __restrict__ cst,
                                                              u64* __restrict__ out) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  const int64_t r = blockIdx.x;
  const int big = k * N;
  if (col > big) return;
  const int64_t q = r / B, x = r - q * B;
  int s = 0;
  while (s + 1 < ns && ends[s] <= x) ++s;
  const XqGrpTenant e = ten[s];
  const int64_t b = x - e.start;
  const int S = N / e.D;
  const int64_t g = b / S;
  const int p = (int)(b - g * S) * e.D;
  const u64* src = Mall + e.m0 + ((size_t)q * (size_t)e.G + (size_t)g) * (k + 1) * N;
  out[(size_t)r * (big + 1) + col] = xq_extract_word(src, p, col, N, k, cst[q]);
}

#if !FHEICP_GRP_XGENS
// -DFHEICP_GRP_XGENS=0 builds: a generation's compact Q x B_g rows (what
// fhe_linear_ggsws_batch writes) into rows q B + off + b of the call's matrix.
// Grid (Q B_g, ceil((kN + 1) / 256)).
__global__ void __launch_bounds__(256) k_xq_gens_scatter(const u64* __restrict__ src, int64_t Bg, int64_t off,
                                                         int64_t B, int n1, u64* __restrict__ out) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  if (col >= n1) return;
  const int64_t r = blockIdx.x, q = r / Bg, b = r - q * Bg;
  out[(size_t)(q * B + off + b) * n1 + col] = src[(size_t)r * n1 + col];
}
#endif
