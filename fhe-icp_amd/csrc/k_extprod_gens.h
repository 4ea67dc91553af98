// The transposed external product over the key generations of ONE context
// (DESIGN.md §8.19). Included by fheicp.hip after k_extprod_grp.h.
//
// After a key rotation the documents of several generations are resident, each
// generation's under its own big key, and the client sends every query once
// per generation. Generation g's documents meet generation g's GGSWs: a
// generation is a "tenant" of k_extprod_grp.h's tables, with the same Q and D
// as every other and its own GGSWs, document operand and result M_g. The plane
// and the MFMA kernels of the group form run as they are; what differs is the
// output: not the group's padded per-tenant segments but ONE query-major
// Q x B matrix (row q B + off_g + b, off_g the documents before generation g),
// the layout the segmented bridge (k_bridge.h) takes its row map over.
//
// A segment is a generation with documents; XqGrpTenant.start holds off_g.
#pragma once

constexpr int XQ_GENS_MAX = FHE_BRIDGE_SLOTS + 1;  // every bridge slot's generation and the current one
struct XqGensSegs {
  XqGrpTenant v[XQ_GENS_MAX];
};

// The tables of a call, one thread per entry of the longest: the records, tile
// -> (segment, column workgroup, row-tile group), row tile -> segment (every
// segment has the same rtp padded row tiles: one Q), and the segments' document
// ends for the extraction. No quad table: a row finds its segment by its
// document index.
__global__ void __launch_bounds__(256) k_xq_gens_tables(XqGensSegs h, int ns, int N, int RT, int64_t rtp,
                                                        int64_t ntiles, XqGrpTenant* __restrict__ ten,
                                                        XqGrpTile* __restrict__ tiles,
                                                        int32_t* __restrict__ rt_tenant, int64_t* __restrict__ ends) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ns) {
    ten[i] = h.v[i];
    ends[i] = h.v[i].start + h.v[i].B;
  }
  if (i < ntiles) {
    int64_t t0 = 0;
    for (int u = 0; u < ns; ++u) {
      const int64_t cg = xq_grp_cgrid(N, h.v[u].G), n = cg * (rtp / RT);
      if (i < t0 + n) {
        const int64_t loc = i - t0;
        tiles[i] = {u, (int32_t)(loc % cg), (int32_t)(loc / cg), 0};
        break;
      }
      t0 += n;
    }
  }
  if (i < ns * rtp) rt_tenant[i] = (int32_t)(i / rtp);
}

// k_extprod_extract_queries over the Q x B rows of all segments: row
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
  u64 v;
  if (col == big) {
    v = src[(size_t)k * N + p] + cst[q];
  } else {
    const int c = col / N, u = col - c * N;
    v = u <= p ? src[(size_t)c * N + p - u] : (u64)0 - src[(size_t)c * N + p - u + N];
  }
  out[(size_t)r * (big + 1) + col] = v;
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
