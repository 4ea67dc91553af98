// libfheicp: MI355X-native TFHE engine for the encrypted pairwise compare of
// shipstone-labs/fhe-icp. C ABI in include/fhe_icp.h; design in DESIGN.md.
//
// One translation unit, so the whole engine is one gfx950 code object:
//   common.h          device helpers (modulus switch, gadget digits, test vectors)
//   k_client.h        keygen, encrypt / decrypt, seeded (stored) corpus kernels
//   k_server.h        leveled linear layer, key switch (VALU and i8 MFMA),
//                     quantisation, top-k
//   k_ks_grp.h        group form of the i8 MFMA key switch: block table, digits
//                     and GEMM over several key holders' rows
//   k_query.h         private-query search: document packing, query byte planes,
//                     the i8 MFMA GEMM of one encrypted query x clear documents
//   k_pack.h          LWE -> GLWE packing key switch (two-party replies): wide
//                     digits, key generation, rotation, packed decryption
//   k_bridge.h        LWE -> LWE bridge key switch (key rotation of stored
//                     ciphertexts): key generation, mapped digits and scatter
//                     for one key's rows and for segments with a key each
//                     (several old generations, every tenant of a group)
//   k_extprod.h       both-private search: GGSW query encryption, GLWE document
//                     digits, Toeplitz byte planes, slot extraction
//   k_extprod_q.h     both-private search, Q queries in one pass: reversed
//                     document digits, GGSW byte planes, the transposed i8 GEMM
//   k_extprod_grp.h   the same over the segments of a call (the tenants of a
//                     group, the key generations of a context): one table kernel
//   k_private_seeded.h  both-private search on seeded documents and queries
//   k_seeded_keys.h   seeded evaluation keys: LWE-row expansion, body gather
//   k_blind_rotate.h  blind rotation (external products over an f64 wave FFT):
//                     v4 (br_v4.h, the default hot kernel), v2/v3, v1
//   this file         context, launch selection, profiling, the C ABI
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fhe_icp.h"
#include "../../include/fhe_icp_dev.h"
#include "common.h"
#include "k_client.h"
#include "k_server.h"
#include "k_ks_grp.h"
#include "k_query.h"
#include "k_pack.h"
#include "k_bridge.h"
#include "k_extprod.h"
#include "k_extprod_q.h"
#include "k_private_seeded.h"
#include "k_seeded_keys.h"
#include "k_blind_rotate.h"
#ifndef FHEICP_GRP_XGENS
#define FHEICP_GRP_XGENS 1  // 0: one fhe_linear_ggsws_batch per generation and a scatter behind the same entries
                            // (A/B builds, tools/build_variant.sh NAME -DFHEICP_GRP_XGENS=0)
#endif
#include "k_extprod_grp.h"

// ============================================================ host =========
struct ProfAcc {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double ms = 0;
  int64_t launches = 0, items = 0;
  const char* kernel = nullptr;  // the last launched instantiation (rocprofv3's name)
};

// a device workspace grown on demand (reserve below)
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
// a gadget key switch's key (k_pack.h, k_bridge.h): gadget (beta, level), the
// key [i][l][n1] as exported and its 8 byte planes in B-fragment order. A
// level of 0: no key in place.
struct GadgetKey {
  u64* key = nullptr;
  int8_t* planes = nullptr;
  int beta = 0, level = 0;
  bool seeded = false;  // the masks are the streams of `mask` (§8.16): the key can be exported seeded
  ChaKey mask{};
  bool keyed = false;   // generated unseeded with the key `gen` (the bridge slots' courtesy check, §8.17)
  ChaKey gen{};
};

struct fhe_ctx;
static void prof_begin(fhe_ctx* ctx, ProfAcc& a, hipStream_t st, hipEvent_t* e1);
static void prof_end(fhe_ctx* ctx, ProfAcc& a, hipStream_t st, hipEvent_t e1, int64_t items);

struct fhe_ctx {
  fhe_params p{};
  int device = -1;
  std::string err;
  bool keys = false;    // evaluation keys (bsk, ksk, the gadgets' keys) are in place
  bool secret = false;  // ... and the secret keys: false after fhe_import_eval_keys
  u64 *s_small = nullptr, *s_big = nullptr, *bsk = nullptr, *ksk = nullptr, *ksk_colsum = nullptr;
  c64 *bsk_fft = nullptr, *tw = nullptr, *twist = nullptr, *tw4 = nullptr;
  c64* bsk_fft_v2 = nullptr;  // v2-layout copy of the main BSK for the table bootstrap (made on first use)
  // bootstrapping keys of the other gadgets (g = 1..5: p.pbs_fast_*,
  // pbs_fast2_*, pbs_mid_*, pbs_mid2_*, pbs_mid0_*), coefficient domain and FFT form
  u64* bskf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  c64* bskf_fft[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // multi-bit blind rotation of the fast gadgets with pbs_fast*_group = 2
  // (DESIGN.md §4.5): their keys hold three GGSWs per pair of LWE
  // coefficients (messages in mb_msg); psi^x table, x < 2N (bank-swizzled)
  c64* psi = nullptr;
  u64* mb_msg = nullptr;
  int mb_dbg = 0;      // A/B builds: FHEICP_MB_DBG timing variants of the multi-bit kernel
  int v4s = 0;         // A/B builds: FHEICP_V4S=1, key-stationary v4s for the 32-bit kernels too
  // workspace
  DevBuf ws;
  bool prof = false;
  ProfAcc prof_br, prof_brf[5], prof_ks;  // blind rotation on the main / fast / fast2 / mid / mid2 / mid0 gadget
  ProfAcc prof_enc;                       // the fused client encryption + leveled dot (k_encrypt_linear)
  ProfAcc prof_lq;                        // private-query leveled step: k_query_planes + k_linear_query_mfma
  DevBuf lq_ws;                           // its query byte planes (grown on demand)
  ProfAcc prof_ls;                        // stored-ciphertext leveled step, batched: k_linear_seeded_queries
  DevBuf lsq_cst;                         // fhe_linear_seeded_queries_batch's Q scaled constants (grown on demand)
  int br_variant = 4;  // N=1024 blind rotation: 4 = a wave per GLWE component (k = 2, default), 2
                       // (two waves per ciphertext; forced by FHEICP_BR_VARIANT=2)
  // A/B builds only (FHEICP_AB, tools/build_variant.sh): other v4 shapes
  int v4_g = 4;        // v4 ciphertexts per workgroup (FHEICP_V4_G = 1, 2 or 4)
  int v4_fl = 0;       // v4 per-ciphertext LDS hand-offs instead of s_barrier (FHEICP_V4_FL=1)
  int v4_a64 = 0;      // v4: 64-bit accumulators even where 32 bits suffice (FHEICP_V4_A64=1)
  int v4_dbg = 0;      // timing experiments only (FHEICP_V4_DBG), wrong results
  // i8-MFMA key switch: key byte planes and a digit/body workspace
  int8_t* ksk8 = nullptr;
  DevBuf ks_ws[2];  // lane 0 (every caller stream) and lane 1: the second half of a pipelined compare
  // two streams and their events for the pipelined sign extraction of
  // fhe_compare_batch (created on first use)
  hipStream_t lane_st[2] = {nullptr, nullptr};
  hipEvent_t lane_ev[3] = {nullptr, nullptr, nullptr};
  int ks_variant = 2;  // 2 = MFMA (i8 planes, any ks_level with kN % 64 == 0), 1 = VALU split-K
  // LWE -> GLWE packing key (k_pack.h), (k+1)N columns
  GadgetKey pack_key;
  DevBuf pack_ws;           // digits | zero bodies | the GEMM's count x (k+1)N result
  ProfAcc prof_pack;        // fhe_pack_batch: k_pack_digits + the GEMM + k_pack_rotate
  // LWE -> LWE bridge keys of a key rotation (k_bridge.h), kN + 1 columns:
  // slot 0 is the bridge key of §8.12, the others serve further old
  // generations (§8.17)
  GadgetKey bridge_keys[FHE_BRIDGE_SLOTS];
  DevBuf bridge_ws;         // (a segmented pass's tables |) digits | bodies | the GEMM's count x (kN+1) compact result
  ProfAcc prof_bridge;      // fhe_bridge_batch: k_bridge_digits + the GEMM + k_bridge_scatter
  // both-private search (k_extprod.h): the query's Toeplitz byte planes |
  // zero bodies | the GEMM's G x (k+1)N result, allocated on first use
  DevBuf xp_ws;
  ProfAcc prof_xp;          // fhe_linear_ggsw_batch: k_extprod_planes + the GEMM + k_extprod_extract
  // the batched entries (k_extprod_q.h) use xp_ws as: the Q queries' byte
  // planes | the Q x G x (k+1)N result | the Q scaled constants
  ProfAcc prof_xq;          // fhe_linear_ggsws_batch: k_ggsws_planes + the GEMM + k_extprod_extract_queries
  // seeded GGSW queries (k_private_seeded.h): their full form, Q x fhe_ggsw_words
  // (grown on demand), and the time of k_expand_ggsw_seeded
  DevBuf xs_ws;
  ProfAcc prof_xs;
  // seeded evaluation keys (k_seeded_keys.h): the public mask
  // key of bsk and ksk (eval_seeded) and of the other gadgets' keys
  // (fast_seeded: fhe_import_keys re-encrypts those under a private key), every
  // mask key a seeded keygen of this context has used, and the bodies' staging
  // buffer of an export or import (freed when the entry returns)
  bool eval_seeded = false, fast_seeded = false;
  ChaKey eval_mask{};
  std::vector<ChaKey> used_masks;
  DevBuf sk_ws;
};

static std::mutex g_err_mu;
static std::string g_err;

static int fail(fhe_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = msg;
  return code;
}
#define HIPCHK(ctx, x)                                                                          \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) return fail(ctx, FHE_E_DEVICE, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

// Grows `b` to at least `bytes`; what it held is lost. A grow synchronises the
// device before it frees (work queued on any stream may still read the old
// buffer). The record is empty while the allocation is in flight, so a failed
// one leaves it empty and the next call allocates again. The allocation's
// failure returns the caller's code and message (ctx == nullptr: a group's,
// the message with its "group: " prefix) and clears HIP's error.
static int reserve(fhe_ctx* ctx, DevBuf& b, size_t bytes, int code, const char* msg) {
  if (bytes <= b.bytes) return FHE_OK;
  if (b.p) {
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipFree(b.p));
  }
  b = DevBuf{};
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return fail(ctx, code, msg);
  }
  b.bytes = bytes;
  return FHE_OK;
}

static int ilog2i(int x) {
  int r = 0;
  while ((1 << r) < x) ++r;
  return r;
}

static int validate(const fhe_params* p, std::string& why) {
  if (!p) { why = "null params"; return -1; }
  if (p->struct_size != FHE_PARAMS_SIZE) {
    why = "fhe_params.struct_size is " + std::to_string(p->struct_size) + ", this library's fhe_params has " +
          std::to_string(FHE_PARAMS_SIZE) + " bytes: the caller was built against another include/fhe_icp.h";
    return -1;
  }
  if (!(p->N == 256 || p->N == 512 || p->N == 1024 || p->N == 2048)) { why = "N must be 256/512/1024/2048"; return -1; }
  if (p->k < 1 || p->k > 2) { why = "k must be 1 or 2"; return -1; }
  if (p->N == 2048 && p->k != 1) { why = "N=2048 requires k=1"; return -1; }
  if (p->n < 1 || p->n > 4096) { why = "n out of range"; return -1; }
  if (p->pbs_level < 1 || p->pbs_level > 8 || p->pbs_base_log < 1 || p->pbs_level * p->pbs_base_log > 62) {
    why = "pbs decomposition out of range"; return -1;
  }
  if (p->ks_level < 1 || p->ks_level > 8 || p->ks_base_log < 1 || p->ks_base_log > 7 ||
      p->ks_level * p->ks_base_log + p->ks_level > 63) {
    why = "ks decomposition out of range (base_log <= 7 for int8 digits)"; return -1;
  }
  if (p->msg_bits < 2 || p->msg_bits > 40) { why = "msg_bits must be in [2, 40]"; return -1; }
  // the key switch's tie coins are input bits 62 - prec - j (j < ks_level),
  // fair only above the zero bits a shifted input brings in: the sign
  // extraction shifts by up to msg_bits - 1 (sign_rounds)
  if (p->ks_level * p->ks_base_log + p->ks_level + p->msg_bits > 64) {
    why = "ks_level * (ks_base_log + 1) + msg_bits must be <= 64 (key-switch tie coins above every shift)";
    return -1;
  }
  if (p->lwe_noise_bits < 0 || p->lwe_noise_bits > 60 || p->glwe_noise_bits < 0 || p->glwe_noise_bits > 60) {
    why = "noise bits out of range"; return -1;
  }
  if (p->sign_digit_bits != 0 && (p->sign_digit_bits < 3 || p->sign_digit_bits > 4)) {
    why = "sign_digit_bits must be 0 (auto), 3 or 4"; return -1;
  }
  if ((p->pbs_fast_base_log == 0) != (p->pbs_fast_level == 0) || p->pbs_fast_level < 0 || p->pbs_fast_level > 8 ||
      p->pbs_fast_base_log < 0 || p->pbs_fast_level * p->pbs_fast_base_log > 62) {
    why = "fast pbs decomposition out of range (0, 0 for none)"; return -1;
  }
  if ((p->pbs_fast2_base_log == 0) != (p->pbs_fast2_level == 0) || p->pbs_fast2_level < 0 ||
      p->pbs_fast2_level > 8 || p->pbs_fast2_base_log < 0 || p->pbs_fast2_level * p->pbs_fast2_base_log > 62 ||
      (p->pbs_fast2_level && !p->pbs_fast_level)) {
    why = "fast2 pbs decomposition out of range (0, 0 for none; needs a fast gadget)"; return -1;
  }
  if ((p->pbs_mid_base_log == 0) != (p->pbs_mid_level == 0) || p->pbs_mid_level < 0 || p->pbs_mid_level > 8 ||
      p->pbs_mid_base_log < 0 || p->pbs_mid_level * p->pbs_mid_base_log > 62 ||
      (p->pbs_mid_level && !p->pbs_fast_level)) {
    why = "mid pbs decomposition out of range (0, 0 for none; needs a fast gadget)"; return -1;
  }
  if ((p->pbs_mid2_base_log == 0) != (p->pbs_mid2_level == 0) || p->pbs_mid2_level < 0 ||
      p->pbs_mid2_level > 8 || p->pbs_mid2_base_log < 0 || p->pbs_mid2_level * p->pbs_mid2_base_log > 62 ||
      (p->pbs_mid2_level && !p->pbs_mid_level)) {
    why = "mid2 pbs decomposition out of range (0, 0 for none; needs the mid gadget)"; return -1;
  }
  if ((p->pbs_mid0_base_log == 0) != (p->pbs_mid0_level == 0) || p->pbs_mid0_level < 0 ||
      p->pbs_mid0_level > 8 || p->pbs_mid0_base_log < 0 || p->pbs_mid0_level * p->pbs_mid0_base_log > 62 ||
      (p->pbs_mid0_level && !p->pbs_mid_level)) {
    why = "mid0 pbs decomposition out of range (0, 0 for none; needs the mid gadget)"; return -1;
  }
  for (int g = 1; g <= 5; ++g) {
    const int grp = g == 1 ? p->pbs_fast_group : g == 2 ? p->pbs_fast2_group : g == 3 ? p->pbs_mid_group
                    : g == 4 ? p->pbs_mid2_group : p->pbs_mid0_group;
    const int L = g == 1 ? p->pbs_fast_level : g == 2 ? p->pbs_fast2_level : g == 3 ? p->pbs_mid_level
                  : g == 4 ? p->pbs_mid2_level : p->pbs_mid0_level;
    const int bl = g == 1 ? p->pbs_fast_base_log : g == 2 ? p->pbs_fast2_base_log
                   : g == 3 ? p->pbs_mid_base_log : g == 4 ? p->pbs_mid2_base_log : p->pbs_mid0_base_log;
    if (grp < 0 || grp > 2) {
      why = "pbs_fast_group / pbs_fast2_group / pbs_mid_group / pbs_mid2_group / pbs_mid0_group must be 0, 1 or 2";
      return -1;
    }
    // 32-bit accumulators when level <= 2 and level * base_log <= 31, else
    // 48-bit (k_blind_rotate_mb64), whose digits are read as 32-bit fields:
    // base_log <= 31 (a wider digit's f64 products are noise anyway)
    if (grp == 2 && L && !(p->N == 1024 && p->k == 2 && p->n <= 1023 && L <= 8 && bl <= 31)) {
      why = "multi-bit blind rotation (group 2) needs N = 1024, k = 2, n <= 1023, level <= 8, base_log <= 31";
      return -1;
    }
    // the 48-bit words keep bits 16-63: every digit field and the rounding
    // bit 2^(63 - L*beta) must lie there, so L * beta <= 47
    if (grp == 2 && L && !(L <= 2 && L * bl <= 31) && L * bl > 47) {
      why = "multi-bit blind rotation (group 2) on 48-bit accumulators needs level * base_log <= 47";
      return -1;
    }
  }
  return 0;
}

// The bootstrap gadgets of a parameter set: 0 main (pbs_base_log,
// pbs_level), 1 fast, 2 fast2, 3 mid, 4 mid2, 5 mid0 (0 levels: absent).
constexpr int NGAD = 6;
static int gadget_level(const fhe_params& p, int g) {
  switch (g) {
    case 0: return p.pbs_level;
    case 1: return p.pbs_fast_level;
    case 2: return p.pbs_fast2_level;
    case 3: return p.pbs_mid_level;
    case 4: return p.pbs_mid2_level;
    case 5: return p.pbs_mid0_level;
  }
  return 0;
}
static int gadget_base_log(const fhe_params& p, int g) {
  switch (g) {
    case 0: return p.pbs_base_log;
    case 1: return p.pbs_fast_base_log;
    case 2: return p.pbs_fast2_base_log;
    case 3: return p.pbs_mid_base_log;
    case 4: return p.pbs_mid2_base_log;
    case 5: return p.pbs_mid0_base_log;
  }
  return 0;
}
// grouping factor of gadget g's blind rotation (the main gadget is classic)
static int gadget_group(const fhe_params& p, int g) {
  const int v = g == 1 ? p.pbs_fast_group : g == 2 ? p.pbs_fast2_group : g == 3 ? p.pbs_mid_group
                : g == 4 ? p.pbs_mid2_group : g == 5 ? p.pbs_mid0_group : 1;
  return v == 2 ? 2 : 1;
}

static double tuniform_var(int b) { return (std::ldexp(1.0, 2 * b + 1) + 1.0) / 6.0; }

// Noise model, the same formulas as fheicp/params.py and
// oracle/tfhe_ref.c; variances relative to the 2^64 torus.
// Bootstrap output variance: key noise + gadget rounding + the f64 FFT's
// arithmetic error (C_FFT = 16 bounds the 11.6-13.8 measured on every kernel
// instance, tests/test_gpu_noise.py) + the 2^32 rounding of the 32-bit
// accumulators (L*beta <= 31), the last two key-weighted per step.
// The multi-bit rotation (group 2): 3x the key noise (three
// GGSWs per pair, each times X^a - 1), the same gadget rounding total, 3x the
// FFT error and half the 2^32 output roundings.
constexpr double C_FFT = 16.0;
static double pbs_var(const fhe_params& p, int beta, int L, int group = 1) {
  const double s2_bsk = tuniform_var(p.glwe_noise_bits) / std::ldexp(1.0, 128);
  const double B = std::ldexp(1.0, beta);
  const double rows = (double)L * (p.k + 1) * p.N;
  const double steps = p.n * (1 + p.k * p.N / 2.0);
  const double fft = C_FFT * rows * B * B / 144.0 * std::ldexp(1.0, -106);
  const double out32 = beta * L <= 31 ? std::ldexp(1.0, -64) / 12.0 : 0.0;
  const double km = group == 2 ? 3.0 : 1.0;
  const double arith = group == 2 ? 3.0 * fft + 0.5 * out32 : fft + out32;
  return km * p.n * rows * (B * B + 2) / 12.0 * s2_bsk + steps / (12.0 * std::pow(B, 2.0 * L)) + steps * arith;
}
// the key switch's KSK words are rounded to multiples of 2^R (k_server.h
// ks_round): R = 8 floor((lwe_noise_bits - 6) / 8), so the rounding's
// 2^R / sqrt(12) stays below 2^-7 of the KSK noise TUniform(lwe_noise_bits)
// and the i8 MFMA key switch runs on 8 - R / 8 byte planes (3 at the shipped
// lwe_noise_bits = 46; R at most 40). oracle/tfhe_ref.c ks_round_bits and
// params.ks_round_bits agree.
static int ks_round_bits(const fhe_params& p) {
  return p.lwe_noise_bits < 14 ? 0 : 8 * std::min((p.lwe_noise_bits - 6) / 8, 5);
}
// the MFMA key switch's column blocks per workgroup (k_keyswitch_mfma CB):
// three when the rounded key has at most 4 byte planes, and the 16-column
// blocks of the key planes padded to a multiple of it (zero columns)
static int ks_cb(const fhe_params& p) { return 8 - ks_round_bits(p) / 8 <= 4 ? 3 : 1; }
static int ks_nb(const fhe_params& p) {
  const int cb = ks_cb(p), nb = (p.n + 1 + KSM_NB_COLS - 1) / KSM_NB_COLS;
  return (nb + cb - 1) / cb * cb;
}
static double ks_var(const fhe_params& p) {
  const int R = ks_round_bits(p);
  const double s2_ksk = (tuniform_var(p.lwe_noise_bits) + (R ? std::ldexp(1.0, 2 * R) / 12.0 : 0.0)) /
                        std::ldexp(1.0, 128);
  const double Bk = std::ldexp(1.0, p.ks_base_log);
  return (double)p.k * p.N * p.ks_level * (Bk * Bk + 2) / 12.0 * s2_ksk +
         p.k * p.N / 2.0 * std::ldexp(1.0, -2 * p.ks_level * p.ks_base_log) / 12.0;
}
// modulus switch to 2N: one rounding per set key bit and the body (classic);
// the multi-bit rotation rounds the active subset's exponent from the exact
// sum (k_blind_rotate.h mb_rotate), one rounding per pair with a set bit
static double ms_var(const fhe_params& p, int group = 1) {
  const double per = group == 2 ? (p.n / 2) * 0.75 / 12.0 + (p.n % 2) * 0.5 / 12.0 + 1.0 / 12.0
                                : (p.n / 2.0 + 1) / 12.0;
  return per / ((2.0 * p.N) * (2.0 * p.N));
}

// Decision margin in sigmas of the worst round of a d-bit digit sign
// extraction on one gadget: the staircase round of the lowest digit, margin
// 2^-(d+1) of the torus, the preceding bootstrap's noise amplified by
// 2^(P-d), plus key switch and modulus switch noise.
static double digit_margin_sigmas(const fhe_params& p, int d) {
  const double v = pbs_var(p, p.pbs_base_log, p.pbs_level) * std::ldexp(1.0, 2 * (p.msg_bits - d)) + ks_var(p) +
                   ms_var(p);
  return std::ldexp(1.0, -(d + 1)) / std::sqrt(v);
}

// The bootstraps of fhe_sign_batch in order, as (shift, log2 margin): the
// round reads v << shift, and every earlier bootstrap output subtracted from
// v is amplified by 2^shift.
static int sign_rounds(int P, int d, int* shift, int* mlog) {
  int R = 0, b = 0;
  const int m = P - d;
  auto add = [&](int sh, int ml) { shift[R] = sh; mlog[R] = ml; ++R; };
  for (; b + d <= m; b += d) { add(P - b - d, -(d + 1)); add(P - b - d, -(d + 1)); }
  if (m - b >= 3) { const int c = m - b; add(P - b - c, -(c + 1)); add(P - b - c, -(c + 1)); b = m; }
  for (; b < m; ++b) add(P - b - 1, -2);
  add(0, -(d + 1));
  return R;
}
// worst margin (sigmas) over all R rounds when round r runs on gadget sched[r]
static double plan_worst(const fhe_params& p, int d, const int* sched) {
  int sh[64], ml[64];
  const int R = sign_rounds(p.msg_bits, d, sh, ml);
  double var[NGAD];
  for (int g = 0; g < NGAD; ++g)
    var[g] = gadget_level(p, g) ? pbs_var(p, gadget_base_log(p, g), gadget_level(p, g), gadget_group(p, g)) : 0.0;
  double fixed[NGAD];  // key switch + the modulus switch of each gadget's rotation
  for (int g = 0; g < NGAD; ++g) fixed[g] = ks_var(p) + ms_var(p, gadget_group(p, g));
  double acc = 0, worst = 1e300;
  for (int r = 0; r < R; ++r) {
    worst = std::min(worst, std::ldexp(1.0, ml[r]) / std::sqrt(acc * std::ldexp(1.0, 2 * sh[r]) + fixed[sched[r]]));
    acc += var[sched[r]];
  }
  // the last bootstrap's output is the sign ciphertext: decryptable at 1/4
  return std::min(worst, 0.25 / std::sqrt(var[sched[R - 1]]));
}
// The sign plan: digit width d and the gadget of every
// bootstrap (sched[0..R), returns R). Without a fast gadget: the
// single-gadget rule (d = 4 if its worst round keeps 9.2 sigma, else 3), all
// rounds on the main gadget. With fast gadgets: the widest d (or the forced
// one); then along the ladder main, mid0, mid, mid2, fast, fast2 (those present,
// noisier down the ladder) each gadget takes the fewest leading rounds for
// which the next gadget on all the remaining ones keeps every decision at 9.2
// sigma; the last one takes the rest.
static int sign_schedule(const fhe_params& p, int* d_out, int* sched) {
  int sh[64], ml[64];
  const int P = p.msg_bits;
  if (P < 4) {
    *d_out = 0;
    for (int r = 0; r < P; ++r) sched[r] = 0;
    return P;
  }
  auto all_main = [&](int d) {
    const int R = sign_rounds(P, d, sh, ml);
    for (int r = 0; r < R; ++r) sched[r] = 0;
    *d_out = d;
    return R;
  };
  if (!p.pbs_fast_level) {
    int d = 3;
    if (p.sign_digit_bits) d = std::min(p.sign_digit_bits, P);
    else if (digit_margin_sigmas(p, std::min(4, P)) >= 9.2) d = std::min(4, P);
    return all_main(d);
  }
  int lad[NGAD], m = 0;
  lad[m++] = 0;
  for (int g : {5, 3, 4, 1, 2})
    if (gadget_level(p, g)) lad[m++] = g;
  const int first = p.sign_digit_bits ? std::min(p.sign_digit_bits, P) : std::min(4, P);
  const int last = p.sign_digit_bits ? first : 3;
  for (int d = first; d >= last; --d) {
    const int R = sign_rounds(P, d, sh, ml);
    int start = 0;
    bool ok = true;
    for (int i = 0; i + 1 < m; ++i) {
      int c = start;
      for (; c <= R; ++c) {
        for (int r = start; r < R; ++r) sched[r] = r < c ? lad[i] : lad[i + 1];
        if (plan_worst(p, d, sched) >= 9.2) break;
      }
      if (c > R) {  // only when the main gadget alone cannot: a narrower d
        ok = false;
        break;
      }
      start = c;
    }
    if (ok) {
      *d_out = d;
      return R;
    }
  }
  return all_main(last);
}
// (d, j1, j2): digit width, the leading main-gadget rounds and the first
// fast2 round (R without one) of sign_schedule
static void sign_plan(const fhe_params& p, int* d_out, int* j1_out, int* j2_out) {
  int sched[64];
  const int R = sign_schedule(p, d_out, sched);
  int j1 = 0, j2 = R;
  while (j1 < R && sched[j1] == 0) ++j1;
  while (j2 > 0 && sched[j2 - 1] == 2) --j2;
  *j1_out = j1;
  *j2_out = j2;
}
static int sign_digits(const fhe_params& p) {
  int d, j1, j2;
  sign_plan(p, &d, &j1, &j2);
  return d;
}

// The K split of the i8 MFMA key-switch GEMM (k_keyswitch_mfma and its group
// form) over S workgroups when the `ktiles` of its (ciphertext block, column
// group) grid alone would leave CUs idle: towards `target` workgroups, ~2 per
// CU (S = 3 at 1024 ciphertexts; 1, 2, 4-12 measured slower there,
// tools/ks_sweep.py). Slices are whole ring rounds, so every slice holds at
// least KSM_RING k-blocks for the kernel's prologue; the partial sums meet by
// 64-bit atomics in a zeroed result. `force` > 0 (A/B builds) sets S instead.
struct KsmSplit {
  int S, kslice;
};
static KsmSplit ksm_split(int KB, int64_t ktiles, int64_t target, int force = 0) {
  int S = (int)std::max<int64_t>(1, std::min<int64_t>(KB / KSM_RING, target / std::max<int64_t>(1, ktiles)));
  if (force > 0) S = std::max(1, std::min(KB / KSM_RING, force));
  const int kslice = (KB / KSM_RING + S - 1) / S * KSM_RING;
  return {(KB + kslice - 1) / kslice, kslice};
}
// The instantiated (byte planes Q, column blocks CB) pairs of those two
// kernels: f(Q, CB) with both as compile-time constants; false for any other pair.
template <class F>
static bool ksm_dispatch(int planes, int CB, F&& f) {
#define KSM_PAIR(Q, C) \
  case Q * 4 + C: f(std::integral_constant<int, Q>{}, std::integral_constant<int, C>{}); return true
  switch (planes * 4 + CB) {
    KSM_PAIR(3, 3);
    KSM_PAIR(4, 3);
    KSM_PAIR(5, 1);
    KSM_PAIR(6, 1);
    KSM_PAIR(7, 1);
    KSM_PAIR(8, 1);
    default: return false;
  }
#undef KSM_PAIR
}
// rocprofv3's name of an instantiation, for a profile bucket: "base<Q, C>"
static std::string ksm_name(const char* base, int Q, int C) {
  return std::string(base) + "<" + std::to_string(Q) + ", " + std::to_string(C) + ">";
}
// The transposed external product's K split (k_extprod_q.h, k_extprod_grp.h)
// over workgroups, towards ~XQ_WGS of them on the launch's `tiles` (column
// workgroups x row-tile groups), slices of 4 k-blocks at least.
#ifndef FHEICP_XQ_WGS
#define FHEICP_XQ_WGS 512  // A/B builds (tools/build_variant.sh): other targets
#endif
static KsmSplit xq_ksplit(int KB, int64_t tiles) {
  const int S = (int)std::max<int64_t>(1, std::min<int64_t>(KB / 4, FHEICP_XQ_WGS / std::max<int64_t>(1, tiles)));
  const int kslice = (KB + S - 1) / S;
  return {(KB + kslice - 1) / kslice, kslice};
}
// Its GEMMs' row tiles per workgroup, RT = 1 or 2: f(RT) with RT as a compile-time constant.
template <class F>
static void xq_dispatch(int RT, F&& f) {
  if (RT == 2)
    f(std::integral_constant<int, 2>{});
  else
    f(std::integral_constant<int, 1>{});
}

extern "C" {

size_t fhe_bsk_words(const fhe_params* p) {
  return (size_t)p->n * (p->k + 1) * p->pbs_level * (p->k + 1) * p->N;
}
size_t fhe_ksk_words(const fhe_params* p) { return (size_t)p->k * p->N * p->ks_level * (p->n + 1); }
size_t fhe_big_lwe_words(const fhe_params* p) { return (size_t)p->k * p->N + 1; }
size_t fhe_small_lwe_words(const fhe_params* p) { return (size_t)p->n + 1; }

const char* fhe_last_error(const fhe_ctx* ctx) {
  if (ctx) return ctx->err.c_str();
  std::lock_guard<std::mutex> lk(g_err_mu);
  return g_err.c_str();
}

int fhe_get_params(const fhe_ctx* ctx, fhe_params* out) {
  if (!ctx || !out) return FHE_E_ARG;
  *out = ctx->p;
  return FHE_OK;
}

int fhe_ctx_create(const fhe_params* params, int device, fhe_ctx** out) {
  std::string why;
  if (!out) return fail(nullptr, FHE_E_ARG, "out is null");
  *out = nullptr;
  if (validate(params, why)) return fail(nullptr, FHE_E_ARG, why);
  fhe_ctx* ctx = new fhe_ctx();
  ctx->p = *params;
  ctx->device = device;
  if (const char* e = getenv("FHEICP_BR_VARIANT")) {
    const int v = atoi(e);
    ctx->br_variant = (v == 2 || v == 4) ? v : 4;
  }
#ifdef FHEICP_AB
  if (const char* e = getenv("FHEICP_V4_DBG")) ctx->v4_dbg = atoi(e);
  if (const char* e = getenv("FHEICP_V4_G")) {
    const int g = atoi(e);
    ctx->v4_g = (g == 1 || g == 2 || g == 4) ? g : 4;
  }
  if (const char* e = getenv("FHEICP_V4_FL")) ctx->v4_fl = atoi(e) != 0;
  if (const char* e = getenv("FHEICP_V4_A64")) ctx->v4_a64 = atoi(e) != 0;
  if (const char* e = getenv("FHEICP_MB_DBG")) ctx->mb_dbg = atoi(e);
  if (const char* e = getenv("FHEICP_V4S")) ctx->v4s = atoi(e);
#endif
  if (const char* e = getenv("FHEICP_KS_VARIANT")) ctx->ks_variant = atoi(e) == 1 ? 1 : 2;
  // the MFMA key switch: digits in i8, K = kN * ks_level level-major in
  // 64-blocks, |sum| <= K * 2^(beta-1) * 128 < 2^31 in the i32 accumulators
  if ((params->k * params->N) % 64 != 0 || params->ks_level * params->ks_base_log > 31 ||
      params->ks_base_log > 8 ||
      (double)params->k * params->N * params->ks_level * std::ldexp(1.0, params->ks_base_log - 1) * 128 >= 2147483648.0)
    ctx->ks_variant = 1;
  // v4 covers k = 2, n <= 1023 at N = 1024; otherwise the two-wave kernel
  // (measured: v4 wins at gadget levels <= 3, e.g. 21.6 vs 23.6 ms at P=21; from
  // level 4 its 64-bit accumulator spills and v2 is faster, 40.6 vs 53.0 ms at P=26)
  // (the choice is per gadget: variant_for)
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
      delete ctx;
      return fail(nullptr, FHE_E_DEVICE, "no HIP device " + std::to_string(device));
    }
    if (hipSetDevice(device) != hipSuccess) {
      delete ctx;
      return fail(nullptr, FHE_E_DEVICE, "hipSetDevice failed");
    }
    const int N = params->N, M = N / 2;
    std::vector<c64> tw(M / 2), twist(M);
    for (int x = 0; x < M / 2; ++x) {
      const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)x / (long double)M;
      tw[x] = {(double)cosl(ang), (double)sinl(ang)};
    }
    for (int t = 0; t < M; ++t) {
      const long double ang = 3.14159265358979323846264338327950288L * (long double)t / (long double)N;
      twist[t] = {(double)cosl(ang), (double)sinl(ang)};
    }
    if (N == 1024) {  // v4 per-lane twiddles (br_v4.h), long double
      const long double PI = 3.14159265358979323846264338327950288L;
      std::vector<c64> t4(v4::NTW);
      for (int m = 0; m < 8; ++m)
        for (int lane = 0; lane < 64; ++lane) {
          const long double ang = PI * (long double)lane * (long double)(1 + 4 * m) / 1024.0L;
          t4[m * 64 + lane] = {(double)cosl(ang), (double)sinl(ang)};
        }
      for (int m = 1; m < 8; ++m)
        for (int L = 0; L < 8; ++L) {
          const long double ang = 2.0L * PI * (long double)(L * m) / 64.0L;
          t4[v4::NTA + (m - 1) * 8 + L] = {(double)cosl(ang), (double)sinl(ang)};
        }
      // psi^x - 1, psi = exp(i pi / N), x < 2N: the monomial factors of the multi-bit rotation
      std::vector<c64> ps(2 * N);
      for (int x = 0; x < 2 * N; ++x) {
        const long double ang = PI * (long double)x / (long double)N;
        // psi^x - 1, the factor the products take (cos - 1 = -2 sin^2),
        // bank-swizzled (k_blind_rotate_mb)
        const long double h = sinl(ang / 2);
        ps[mb::psi_pos(x)] = {(double)(-2.0L * h * h), (double)sinl(ang)};
      }
      if (hipMalloc(&ctx->tw4, sizeof(c64) * t4.size()) != hipSuccess ||
          hipMemcpy(ctx->tw4, t4.data(), sizeof(c64) * t4.size(), hipMemcpyHostToDevice) != hipSuccess ||
          hipMalloc(&ctx->psi, sizeof(c64) * ps.size()) != hipSuccess ||
          hipMemcpy(ctx->psi, ps.data(), sizeof(c64) * ps.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fhe_ctx_destroy(ctx);
        return fail(nullptr, FHE_E_DEVICE, "twiddle upload failed");
      }
    }
    if (hipMalloc(&ctx->tw, sizeof(c64) * tw.size()) != hipSuccess ||
        hipMalloc(&ctx->twist, sizeof(c64) * twist.size()) != hipSuccess ||
        hipMemcpy(ctx->tw, tw.data(), sizeof(c64) * tw.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ctx->twist, twist.data(), sizeof(c64) * twist.size(), hipMemcpyHostToDevice) != hipSuccess) {
      fhe_ctx_destroy(ctx);
      return fail(nullptr, FHE_E_DEVICE, "table upload failed");
    }
  }
  *out = ctx;
  return FHE_OK;
}

static void free_ev(ProfAcc& a) {
  for (auto& e : a.ev) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  a.ev.clear();
}

void fhe_ctx_destroy(fhe_ctx* ctx) {
  if (!ctx) return;
  if (ctx->device >= 0) {
    // teardown: nothing useful can be done about a failed free
    (void)hipSetDevice(ctx->device);
    for (void* ptr : {(void*)ctx->s_small, (void*)ctx->s_big, (void*)ctx->bsk, (void*)ctx->ksk,
                      (void*)ctx->ksk_colsum, (void*)ctx->bsk_fft, (void*)ctx->tw, (void*)ctx->twist, ctx->ws.p,
                      (void*)ctx->bskf[0], (void*)ctx->bskf[1], (void*)ctx->bskf_fft[0], (void*)ctx->bskf_fft[1],
                      (void*)ctx->bskf[2], (void*)ctx->bskf[3], (void*)ctx->bskf_fft[2], (void*)ctx->bskf_fft[3],
                      (void*)ctx->bskf[4], (void*)ctx->bskf_fft[4],
                      (void*)ctx->ksk8, ctx->ks_ws[0].p, ctx->ks_ws[1].p, (void*)ctx->tw4, (void*)ctx->bsk_fft_v2,
                      (void*)ctx->psi, (void*)ctx->mb_msg, ctx->lq_ws.p, (void*)ctx->pack_key.key,
                      (void*)ctx->pack_key.planes, ctx->pack_ws.p, ctx->xp_ws.p, ctx->xs_ws.p, ctx->lsq_cst.p, ctx->sk_ws.p,
                      ctx->bridge_ws.p})
      (void)hipFree(ptr);
    for (GadgetKey& k : ctx->bridge_keys) {
      (void)hipFree(k.key);
      (void)hipFree(k.planes);
    }
    for (hipStream_t s : ctx->lane_st)
      if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : ctx->lane_ev)
      if (e) (void)hipEventDestroy(e);
    free_ev(ctx->prof_br);
    for (auto& a : ctx->prof_brf) free_ev(a);
    free_ev(ctx->prof_ks);
    free_ev(ctx->prof_enc);
    free_ev(ctx->prof_lq);
    free_ev(ctx->prof_ls);
    free_ev(ctx->prof_pack);
    free_ev(ctx->prof_bridge);
    free_ev(ctx->prof_xp);
    free_ev(ctx->prof_xq);
    free_ev(ctx->prof_xs);
  }
  delete ctx;
}

int fhe_set_msg_bits(fhe_ctx* ctx, int32_t msg_bits) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  fhe_params q = ctx->p;
  q.msg_bits = msg_bits;
  std::string why;
  if (validate(&q, why)) return fail(ctx, FHE_E_ARG, why);
  ctx->p = q;
  return FHE_OK;
}

static int need_device(fhe_ctx* ctx) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (ctx->device < 0) return fail(ctx, FHE_E_DEVICE, "host-only context");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, FHE_E_DEVICE, "hipSetDevice failed");
  return FHE_OK;
}
// evaluation keys: everything the server side computes with
static int need_eval_keys(fhe_ctx* ctx) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!ctx->keys) return fail(ctx, FHE_E_STATE, "no keys: call fhe_keygen, fhe_import_keys or fhe_import_eval_keys");
  return FHE_OK;
}
// the secret keys too: encryption, decryption, key generation from them
static int need_secret(fhe_ctx* ctx) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (!ctx->secret)
    return fail(ctx, FHE_E_STATE, "no secret key: this context holds evaluation keys only (fhe_import_eval_keys)");
  return FHE_OK;
}

// blind-rotation kernel for a gadget: the requested variant (4 unless
// FHEICP_BR_VARIANT), falling back to v2 where v4 does not apply
// the v4 kernel keeps 32-bit accumulators for this gadget
// (the shipped 32-bit kernels exist for levels 1 and 2 only: a level-3
// gadget with L*beta <= 31, e.g. (10,3), runs on the 64-bit v4s<3> kernel,
// whose noise the model's 2^32 rounding term then over-counts)
static bool v4_a32(const fhe_ctx* ctx, const fhe_params& q) {
  return q.pbs_level <= 2 && q.pbs_level * q.pbs_base_log <= 31 && !ctx->v4_a64;
}

static int variant_for(const fhe_ctx* ctx, const fhe_params& q) {
  // v4 layout: the v4 kernels (32-bit accumulators, L <= 2) and the v4s
  // ones (64-bit accumulators, L <= 8)
  const int lmax = v4_a32(ctx, q) ? 2 : 8;
  if (ctx->br_variant == 4 &&
      !(q.k == 2 && q.n <= v4::NMAX && q.pbs_level <= lmax && (q.pbs_level == 1 || q.pbs_base_log <= 16)))
    return 2;
  return ctx->br_variant;
}
// the parameters seen through gadget g (1: pbs_fast_*, 2: pbs_fast2_*, 3:
// pbs_mid_*, 4: pbs_mid2_*, 5: pbs_mid0_*; same secret keys, other decomposition and
// bootstrapping key)
static int fast_level(const fhe_params& p, int g) { return g >= 1 && g < NGAD ? gadget_level(p, g) : 0; }
// fast gadget g runs the multi-bit blind rotation
static bool mb_for(const fhe_params& p, int g) { return g > 0 && fast_level(p, g) && gadget_group(p, g) == 2; }
static fhe_params fast_params(const fhe_params& p, int g) {
  fhe_params q = p;
  q.pbs_base_log = gadget_base_log(p, g);
  q.pbs_level = fast_level(p, g);
  return q;
}
// GGSWs of a fast gadget's key: one per LWE coefficient, or three per pair
static int fast_ggsws(const fhe_params& p, int g) { return mb_for(p, g) ? 3 * ((p.n + 1) / 2) : p.n; }
static size_t fast_bsk_words(const fhe_params& p, int g) {
  return (size_t)fast_ggsws(p, g) * (p.k + 1) * fast_level(p, g) * (p.k + 1) * p.N;
}
size_t fhe_fast_bsk_words(const fhe_params* p, int32_t which) {
  if (!p || which < 1 || which >= NGAD || !fast_level(*p, which)) return 0;
  return fast_bsk_words(*p, which);
}
// the other gadgets' keys under the ChaCha20 streams 9/10 (fast), 11/12
// (fast2), 17/18 (mid), 19/20 (mid2) and 25/26 (mid0); 13/14, 15/16, 21/22,
// 23/24 and 27/28 for those gadgets' multi-bit keys, whose GGSW messages
// k_mb_msgs derives
static const uint32_t kTagMask[NGAD] = {TAG_BSK_MASK, TAG_BSK2_MASK, TAG_BSK3_MASK, TAG_BSK4_MASK, TAG_BSK5_MASK,
                                        TAG_BSK6_MASK};
static const uint32_t kTagNoise[NGAD] = {TAG_BSK_NOISE, TAG_BSK2_NOISE, TAG_BSK3_NOISE, TAG_BSK4_NOISE, TAG_BSK5_NOISE,
                                         TAG_BSK6_NOISE};
static const uint32_t kTagMbMask[NGAD] = {0, TAG_MB2_MASK, TAG_MB3_MASK, TAG_MB4_MASK, TAG_MB5_MASK, TAG_MB6_MASK};
static const uint32_t kTagMbNoise[NGAD] = {0, TAG_MB2_NOISE, TAG_MB3_NOISE, TAG_MB4_NOISE, TAG_MB5_NOISE, TAG_MB6_NOISE};
static void keygen_fast_bsks(fhe_ctx* ctx, const ChaKey& Km, const ChaKey& Kn, hipStream_t st, int msg_body = 0) {
  const fhe_params& p = ctx->p;
  const size_t shm = 8 * (size_t)p.N + p.N;
  for (int g = 1; g < NGAD; ++g) {
    if (!fast_level(p, g)) continue;
    const fhe_params q = fast_params(p, g);
    const bool mb = mb_for(p, g);
    if (mb) hipLaunchKernelGGL(k_mb_msgs, dim3((q.n + 255) / 256), dim3(256), 0, st, ctx->s_small, q.n, ctx->mb_msg);
    hipLaunchKernelGGL(k_keygen_bsk, dim3(fast_ggsws(p, g) * (q.k + 1) * q.pbs_level), dim3(256), shm, st, Km, Kn,
                       q.N,
                       q.k, q.pbs_level, q.pbs_base_log, q.glwe_noise_bits, mb ? ctx->mb_msg : ctx->s_small,
                       ctx->s_big, ctx->bskf[g - 1],
                       mb ? kTagMbMask[g] : kTagMask[g], mb ? kTagMbNoise[g] : kTagNoise[g], msg_body);
  }
}
// Device buffers of the keys: the evaluation keys always, the secrets (and
// mb_msg, derived from s_small) only with_secret: an evaluation-only context
// never allocates them.
static int alloc_keys(fhe_ctx* ctx, bool with_secret = true) {
  const fhe_params& p = ctx->p;
  for (int g = 1; g < NGAD; ++g) {
    if (!fast_level(p, g)) continue;
    if (!ctx->bskf[g - 1]) {
      HIPCHK(ctx, hipMalloc(&ctx->bskf[g - 1], 8 * fast_bsk_words(p, g)));
      HIPCHK(ctx, hipMalloc(&ctx->bskf_fft[g - 1], sizeof(c64) * fast_bsk_words(p, g) / 2));
    }
    if (with_secret && mb_for(p, g) && !ctx->mb_msg)
      HIPCHK(ctx, hipMalloc(&ctx->mb_msg, 8 * 3 * (size_t)((p.n + 1) / 2)));
  }
  if (with_secret && !ctx->s_small) {
    HIPCHK(ctx, hipMalloc(&ctx->s_small, 8 * (size_t)p.n));
    HIPCHK(ctx, hipMalloc(&ctx->s_big, 8 * (size_t)p.k * p.N));
  }
  if (ctx->bsk) return FHE_OK;
  HIPCHK(ctx, hipMalloc(&ctx->bsk, 8 * fhe_bsk_words(&p)));
  HIPCHK(ctx, hipMalloc(&ctx->ksk, 8 * fhe_ksk_words(&p)));
  HIPCHK(ctx, hipMalloc(&ctx->ksk_colsum, 8 * (size_t)(p.n + 1)));
  HIPCHK(ctx, hipMalloc(&ctx->bsk_fft, sizeof(c64) * fhe_bsk_words(&p) / 2));
  return FHE_OK;
}

static void bsk_to_fft(fhe_ctx* ctx, const fhe_params& p, const u64* bsk, c64* bsk_fft, hipStream_t st,
                       size_t words = 0) {
  const int npoly = (int)((words ? words : fhe_bsk_words(&p)) / p.N);
  switch (p.N) {
    case 256: hipLaunchKernelGGL(k_bsk_to_fft<7>, dim3(npoly), dim3(64), 0, st, bsk, npoly, ctx->tw, ctx->twist, bsk_fft); break;
    case 512: hipLaunchKernelGGL(k_bsk_to_fft<8>, dim3(npoly), dim3(64), 0, st, bsk, npoly, ctx->tw, ctx->twist, bsk_fft); break;
    case 1024:
      if (variant_for(ctx, p) == 4 || words)
        hipLaunchKernelGGL(k_bsk_to_fft_v4, dim3(std::min(npoly, 4096)), dim3(64), 0, st, bsk, npoly, ctx->tw4,
                           bsk_fft, 1.0 / 18446744073709551616.0 / (double)(p.N / 2), words && mb_xpose(p.pbs_level) ? 1 : 0);
      else
        hipLaunchKernelGGL(k_bsk_to_fft_mw<V2>, dim3(npoly), dim3(V2::NT), 0, st, bsk, npoly, ctx->tw, ctx->twist, bsk_fft);
      break;
    case 2048: hipLaunchKernelGGL(k_bsk_to_fft<10>, dim3(npoly), dim3(64), 0, st, bsk, npoly, ctx->tw, ctx->twist, bsk_fft); break;
  }
}
static int convert_bsk(fhe_ctx* ctx, hipStream_t st) {
  const fhe_params& p = ctx->p;
  if (ctx->bsk_fft_v2) {  // the table bootstrap's copy of the old key
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipFree(ctx->bsk_fft_v2));
    ctx->bsk_fft_v2 = nullptr;
  }
  const int R = ks_round_bits(p);
  hipLaunchKernelGGL(k_ksk_colsum, dim3((p.n + 1 + 255) / 256), dim3(256), 0, st, ctx->ksk, p.k * p.N * p.ks_level,
                     p.n, R, ctx->ksk_colsum);
  if (ctx->ks_variant == 2) {
    const int K = p.k * p.N * p.ks_level, n1 = p.n + 1, NB = ks_nb(p);
    if (!ctx->ksk8) HIPCHK(ctx, hipMalloc(&ctx->ksk8, (size_t)K * NB * 16 * (8 - R / 8)));
    const int64_t tot = (int64_t)K * NB * 16;
    hipLaunchKernelGGL(k_ksk_to_i8, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, ctx->ksk, K, p.k * p.N,
                       p.ks_level, n1, NB, R, 8 - R / 8, ctx->ksk8);
  }
  bsk_to_fft(ctx, p, ctx->bsk, ctx->bsk_fft, st);
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g))
      bsk_to_fft(ctx, fast_params(p, g), ctx->bskf[g - 1], ctx->bskf_fft[g - 1], st,
                 mb_for(p, g) ? fast_bsk_words(p, g) : 0);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// The whole key set: the secrets from the noise key Kn (its TAG_SK_* streams),
// every key's masks from Km and noise from Kn. Km = Kn, msg_body = 0:
// fhe_keygen_key. msg_body = 1 (the seeded keygen): the bootstrapping keys'
// messages go to the bodies, every mask word is a stream word (k_keygen_bsk).
static int keygen_impl(fhe_ctx* ctx, const ChaKey& Km, const ChaKey& Kn, hipStream_t st, int msg_body) {
  int rc = alloc_keys(ctx);
  if (rc) return rc;
  const fhe_params& p = ctx->p;
  ctx->eval_seeded = ctx->fast_seeded = false;
  const int big = p.k * p.N;
  const int mx = std::max(p.n, big);
  hipLaunchKernelGGL(k_keygen_secrets, dim3((mx + 255) / 256), dim3(256), 0, st, Kn, p.n, big, ctx->s_small, ctx->s_big);
  const int rows_bsk = p.n * (p.k + 1) * p.pbs_level;
  const size_t shm = 8 * (size_t)p.N + p.N;
  hipLaunchKernelGGL(k_keygen_bsk, dim3(rows_bsk), dim3(256), shm, st, Km, Kn, p.N, p.k, p.pbs_level, p.pbs_base_log,
                     p.glwe_noise_bits, ctx->s_small, ctx->s_big, ctx->bsk, (uint32_t)TAG_BSK_MASK,
                     (uint32_t)TAG_BSK_NOISE, msg_body);
  keygen_fast_bsks(ctx, Km, Kn, st, msg_body);
  hipLaunchKernelGGL(k_keygen_ksk, dim3(big * p.ks_level), dim3(256), 0, st, Km, Kn, p.n, p.ks_level, p.ks_base_log,
                     p.lwe_noise_bits, ctx->s_small, ctx->s_big, ctx->ksk);
  HIPCHK(ctx, hipGetLastError());
  rc = convert_bsk(ctx, st);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->keys = true;
  ctx->secret = true;
  return FHE_OK;
}

int fhe_keygen_key(fhe_ctx* ctx, const uint32_t h_key[8], void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!h_key) return fail(ctx, FHE_E_ARG, "null key");
  ChaKey K;
  memcpy(K.w, h_key, 32);
  return keygen_impl(ctx, K, K, (hipStream_t)stream, 0);
}

int fhe_keygen(fhe_ctx* ctx, uint64_t seed, void* stream) {
  ChaKey K = key_from_seed(seed);
  return fhe_keygen_key(ctx, K.w, stream);
}

int fhe_export_keys(fhe_ctx* ctx, uint64_t* h_s_small, uint64_t* h_s_big, uint64_t* h_bsk, uint64_t* h_ksk) {
  int rc = (h_s_small || h_s_big) ? need_secret(ctx) : need_eval_keys(ctx);
  if (rc) return rc;
  const fhe_params& p = ctx->p;
  HIPCHK(ctx, hipDeviceSynchronize());
  if (h_s_small) HIPCHK(ctx, hipMemcpy(h_s_small, ctx->s_small, 8 * (size_t)p.n, hipMemcpyDeviceToHost));
  if (h_s_big) HIPCHK(ctx, hipMemcpy(h_s_big, ctx->s_big, 8 * (size_t)p.k * p.N, hipMemcpyDeviceToHost));
  if (h_bsk) HIPCHK(ctx, hipMemcpy(h_bsk, ctx->bsk, 8 * fhe_bsk_words(&p), hipMemcpyDeviceToHost));
  if (h_ksk) HIPCHK(ctx, hipMemcpy(h_ksk, ctx->ksk, 8 * fhe_ksk_words(&p), hipMemcpyDeviceToHost));
  return FHE_OK;
}

int fhe_export_fast_bsk(fhe_ctx* ctx, int32_t which, uint64_t* h_bsk) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (which < 1 || which >= NGAD)
    return fail(ctx, FHE_E_ARG, "which must be 1 (fast), 2 (fast2), 3 (mid), 4 (mid2) or 5 (mid0)");
  if (!fast_level(ctx->p, which)) return fail(ctx, FHE_E_STATE, "no such fast gadget in these parameters");
  if (!h_bsk) return fail(ctx, FHE_E_ARG, "null buffer");
  const fhe_params q = fast_params(ctx->p, which);
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpy(h_bsk, ctx->bskf[which - 1], 8 * fast_bsk_words(ctx->p, which), hipMemcpyDeviceToHost));
  return FHE_OK;
}

int fhe_import_keys(fhe_ctx* ctx, const uint64_t* h_s_small, const uint64_t* h_s_big, const uint64_t* h_bsk,
                    const uint64_t* h_ksk) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!h_s_small || !h_s_big || !h_bsk || !h_ksk) return fail(ctx, FHE_E_ARG, "all four key buffers are required");
  rc = alloc_keys(ctx);
  if (rc) return rc;
  const fhe_params& p = ctx->p;
  ctx->eval_seeded = ctx->fast_seeded = false;  // masks of unknown origin
  HIPCHK(ctx, hipMemcpy(ctx->s_small, h_s_small, 8 * (size_t)p.n, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->s_big, h_s_big, 8 * (size_t)p.k * p.N, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->bsk, h_bsk, 8 * fhe_bsk_words(&p), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->ksk, h_ksk, 8 * fhe_ksk_words(&p), hipMemcpyHostToDevice));
  if (p.pbs_fast_level) {
    // the fast gadgets' keys are not part of the exported set: re-encrypt
    // them under the imported secrets with fresh randomness
    ChaKey K;
    std::random_device rd;
    for (int i = 0; i < 8; ++i) K.w[i] = rd();
    keygen_fast_bsks(ctx, K, K, nullptr);
    HIPCHK(ctx, hipGetLastError());
  }
  rc = convert_bsk(ctx, nullptr);
  if (rc) return rc;
  HIPCHK(ctx, hipDeviceSynchronize());
  ctx->keys = true;
  ctx->secret = true;
  return FHE_OK;
}

// An evaluation-only import's first step: the context holds no s_small, s_big
// or mb_msg afterwards (zeroed and freed if it had them).
static int drop_secrets(fhe_ctx* ctx) {
  const fhe_params& p = ctx->p;
  ctx->secret = false;
  if (ctx->s_small || ctx->s_big || ctx->mb_msg) {
    HIPCHK(ctx, hipDeviceSynchronize());
    if (ctx->s_small) HIPCHK(ctx, hipMemset(ctx->s_small, 0, 8 * (size_t)p.n));
    if (ctx->s_big) HIPCHK(ctx, hipMemset(ctx->s_big, 0, 8 * (size_t)p.k * p.N));
    if (ctx->mb_msg) HIPCHK(ctx, hipMemset(ctx->mb_msg, 0, 8 * 3 * (size_t)((p.n + 1) / 2)));
    HIPCHK(ctx, hipDeviceSynchronize());
    for (u64** q : {&ctx->s_small, &ctx->s_big, &ctx->mb_msg}) {
      if (*q) HIPCHK(ctx, hipFree(*q));
      *q = nullptr;
    }
  }
  return FHE_OK;
}

// Evaluation keys only (the server of the two-party mode):
// the keys are used as given and nothing is re-encrypted; the context holds
// no s_small, s_big or mb_msg afterwards (zeroed and freed if it had them).
int fhe_import_eval_keys(fhe_ctx* ctx, const uint64_t* h_bsk, const uint64_t* h_ksk,
                         const uint64_t* const h_gadget_bsk[5]) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!h_bsk || !h_ksk) return fail(ctx, FHE_E_ARG, "the bootstrapping and key-switch key buffers are required");
  const fhe_params& p = ctx->p;
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g) && (!h_gadget_bsk || !h_gadget_bsk[g - 1]))
      return fail(ctx, FHE_E_ARG, "missing bootstrapping key of gadget " + std::to_string(g) +
                                      " (these parameters have it)");
  if ((rc = drop_secrets(ctx))) return rc;
  rc = alloc_keys(ctx, false);
  if (rc) return rc;
  ctx->eval_seeded = ctx->fast_seeded = false;  // masks of unknown origin
  HIPCHK(ctx, hipMemcpy(ctx->bsk, h_bsk, 8 * fhe_bsk_words(&p), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->ksk, h_ksk, 8 * fhe_ksk_words(&p), hipMemcpyHostToDevice));
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g))
      HIPCHK(ctx, hipMemcpy(ctx->bskf[g - 1], h_gadget_bsk[g - 1], 8 * fast_bsk_words(p, g), hipMemcpyHostToDevice));
  rc = convert_bsk(ctx, nullptr);
  if (rc) return rc;
  HIPCHK(ctx, hipDeviceSynchronize());
  ctx->keys = true;
  return FHE_OK;
}

// The encryption entry points take the stream key either as 32 bytes
// (fhe_*_key: the product, a fresh CSPRNG key per session) or as a 64-bit
// seed expanded by splitmix64 (reproducible tests and benches only).
static bool key_arg(const uint32_t* h_key, ChaKey& K) {
  if (!h_key) return false;
  memcpy(K.w, h_key, 32);
  return true;
}

static int encrypt_impl(fhe_ctx* ctx, const int64_t* d_msg, int64_t count, const ChaKey& K, uint64_t id0,
                        uint64_t* d_ct, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!d_msg || !d_ct))) return fail(ctx, FHE_E_ARG, "bad encrypt arguments");
  if (count == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipLaunchKernelGGL(k_encrypt, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, K, p.k * p.N, p.msg_bits,
                     p.glwe_noise_bits, ctx->s_big, d_msg, id0, d_ct);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_encrypt_batch(fhe_ctx* ctx, const int64_t* d_msg, int64_t count, uint64_t seed, uint64_t id0,
                      uint64_t* d_ct, void* stream) {
  return encrypt_impl(ctx, d_msg, count, key_from_seed(seed), id0, d_ct, stream);
}
int fhe_encrypt_batch_key(fhe_ctx* ctx, const int64_t* d_msg, int64_t count, const uint32_t h_key[8], uint64_t id0,
                          uint64_t* d_ct, void* stream) {
  ChaKey K;
  if (!key_arg(h_key, K)) return fail(ctx, FHE_E_ARG, "null encryption key");
  return encrypt_impl(ctx, d_msg, count, K, id0, d_ct, stream);
}

// GLWEs per pair of the packed feature encoding (k_client.h)
static int packed_chunks(const fhe_params& p, int32_t D) { return (D + p.N - 1) / p.N; }

// Km: masks, Kn: noise (the full form passes its one key twice); body_only: the
// seeded form's output, B x G x N body words
static int encrypt_packed_impl(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const ChaKey& Km,
                               const ChaKey& Kn, bool body_only, uint64_t id0, uint64_t* d_glwe, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_qx || !d_glwe))) return fail(ctx, FHE_E_ARG, "bad packed-encrypt arguments");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  const int G = packed_chunks(p, D);
  if (B * G > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "packed-encrypt batch too large: split the call");
  const size_t lds = (size_t)p.k * p.N * 9;
  hipLaunchKernelGGL(k_encrypt_packed, dim3((unsigned)(B * G)), dim3(256), lds, (hipStream_t)stream, Km, Kn, p.N,
                     p.k, p.msg_bits, p.glwe_noise_bits, ctx->s_big, d_qx, (int)D, G, id0, d_glwe, (int)body_only);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_encrypt_packed_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, uint64_t seed, uint64_t id0,
                             uint64_t* d_glwe, void* stream) {
  const ChaKey K = key_from_seed(seed);
  return encrypt_packed_impl(ctx, d_qx, B, D, K, K, false, id0, d_glwe, stream);
}
int fhe_encrypt_packed_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const uint32_t h_key[8],
                                 uint64_t id0, uint64_t* d_glwe, void* stream) {
  ChaKey K;
  if (!key_arg(h_key, K)) return fail(ctx, FHE_E_ARG, "null encryption key");
  return encrypt_packed_impl(ctx, d_qx, B, D, K, K, false, id0, d_glwe, stream);
}

int fhe_linear_packed_batch(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t B, int32_t D, const int64_t* d_w,
                            int64_t cst, uint64_t* d_out, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_glwe || !d_w || !d_out))) return fail(ctx, FHE_E_ARG, "bad packed-linear arguments");
  if (B == 0) return FHE_OK;
  if (B > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "packed-linear batch too large: split the call");
  const fhe_params& p = ctx->p;
  hipLaunchKernelGGL(k_linear_packed, dim3((unsigned)B), dim3(256), (size_t)p.k * p.N * 8, (hipStream_t)stream, p.N,
                     p.k, d_glwe, (int)D, packed_chunks(p, D), d_w, ((u64)cst) << (64 - p.msg_bits), d_out);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

static int encrypt_linear_impl(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const ChaKey& K,
                               uint64_t id0, const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_qx || !d_w || !d_out))) return fail(ctx, FHE_E_ARG, "bad encrypt-linear arguments");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  const int G = packed_chunks(p, D);
  if (B > 0x7fffffffLL || B * G > 0x7fffffffffffLL) return fail(ctx, FHE_E_ARG, "encrypt-linear batch too large: split the call");
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_enc, (hipStream_t)stream, &e1);
  ctx->prof_enc.kernel = "k_encrypt_linear";
  // the chunk's mask in its E form (k_client.h el_region): k * 2N * 9 / 8 words
  hipLaunchKernelGGL(k_encrypt_linear, dim3((unsigned)B), dim3(EL_THREADS), (size_t)p.k * el_region(p.N) * 8,
                     (hipStream_t)stream, K, p.N,
                     p.k, p.msg_bits, p.glwe_noise_bits, ctx->s_big, d_qx, (int)D, G, d_w,
                     ((u64)cst) << (64 - p.msg_bits), id0, d_out);
  prof_end(ctx, ctx->prof_enc, (hipStream_t)stream, e1, B);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_encrypt_linear_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, uint64_t seed, uint64_t id0,
                             const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream) {
  return encrypt_linear_impl(ctx, d_qx, B, D, key_from_seed(seed), id0, d_w, cst, d_out, stream);
}
int fhe_encrypt_linear_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const uint32_t h_key[8],
                                 uint64_t id0, const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream) {
  ChaKey K;
  if (!key_arg(h_key, K)) return fail(ctx, FHE_E_ARG, "null encryption key");
  return encrypt_linear_impl(ctx, d_qx, B, D, K, id0, d_w, cst, d_out, stream);
}

static int seeded_args(fhe_ctx* ctx, int64_t B, int32_t D, const void* a, const void* b, const void* c) {
  if (B < 0 || D <= 0 || (B > 0 && (!a || !b || !c))) return fail(ctx, FHE_E_ARG, "bad seeded-corpus arguments");
  if (B * (int64_t)D > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "seeded corpus batch too large (B*D >= 2^31)");
  return FHE_OK;
}

int fhe_encrypt_seeded_batch(fhe_ctx* ctx, const int64_t* d_msg, int64_t B, int32_t D, const uint32_t h_mask_key[8],
                             const uint32_t h_noise_key[8], const uint64_t* d_id0, uint64_t* d_body, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if ((rc = seeded_args(ctx, B, D, d_msg, d_id0, d_body))) return rc;
  if (!h_mask_key || !h_noise_key) return fail(ctx, FHE_E_ARG, "seeded encryption needs both keys");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  ChaKey Km, Kn;
  for (int i = 0; i < 8; ++i) Km.w[i] = h_mask_key[i], Kn.w[i] = h_noise_key[i];
  hipLaunchKernelGGL(k_encrypt_seeded, dim3((unsigned)(B * D)), dim3(256), 0, (hipStream_t)stream, Km, Kn, p.k * p.N,
                     p.msg_bits, p.glwe_noise_bits, ctx->s_big, d_msg, d_id0, (int)D, d_body);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_expand_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                            const uint32_t h_mask_key[8], uint64_t* d_ct, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if ((rc = seeded_args(ctx, B, D, d_body, d_id0, d_ct))) return rc;
  if (!h_mask_key) return fail(ctx, FHE_E_ARG, "missing mask key");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  ChaKey Km;
  for (int i = 0; i < 8; ++i) Km.w[i] = h_mask_key[i];
  hipLaunchKernelGGL(k_expand_seeded, dim3((unsigned)(B * D)), dim3(256), 0, (hipStream_t)stream, Km, p.k * p.N,
                     d_body, d_id0, (int)D, d_ct);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_linear_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                            const uint32_t h_mask_key[8], const int64_t* d_w, int64_t cst, uint64_t* d_out,
                            void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if ((rc = seeded_args(ctx, B, D, d_body, d_id0, d_out))) return rc;
  if (!h_mask_key || (B > 0 && !d_w)) return fail(ctx, FHE_E_ARG, "missing mask key or weights");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  ChaKey Km;
  for (int i = 0; i < 8; ++i) Km.w[i] = h_mask_key[i];
  hipLaunchKernelGGL(k_linear_seeded, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, Km, p.k * p.N, d_body,
                     d_id0, (int)D, d_w, (u64)cst << (64 - p.msg_bits), d_out);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

static int decrypt_mode(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int64_t* d_out, int mode, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!d_ct || !d_out))) return fail(ctx, FHE_E_ARG, "bad decrypt arguments");
  if (count == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipLaunchKernelGGL(k_decrypt, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, p.k * p.N, p.msg_bits,
                     mode, ctx->s_big, d_ct, d_out);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_decrypt_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int64_t* d_out, void* stream) {
  return decrypt_mode(ctx, d_ct, count, d_out, 0, stream);
}
int fhe_decrypt_bits_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int64_t* d_out, void* stream) {
  return decrypt_mode(ctx, d_ct, count, d_out, 1, stream);
}
int fhe_phase_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, uint64_t* d_out, void* stream) {
  return decrypt_mode(ctx, d_ct, count, (int64_t*)d_out, 2, stream);
}

int fhe_linear_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                     uint64_t* d_out, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_ct || !d_w || !d_out))) return fail(ctx, FHE_E_ARG, "bad linear arguments");
  if (B == 0) return FHE_OK;
  if (B > 65535) return fail(ctx, FHE_E_ARG, "linear batch > 65535: split the call");
  const fhe_params& p = ctx->p;
  const int W = p.k * p.N + 1;
  hipLaunchKernelGGL(k_linear, dim3((W + 255) / 256, (unsigned)B), dim3(256), 0, (hipStream_t)stream, d_ct, D, W, d_w,
                     ((u64)cst) << (64 - p.msg_bits), d_out);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

static void prof_begin(fhe_ctx* ctx, ProfAcc& a, hipStream_t st, hipEvent_t* e1) {
  *e1 = nullptr;
  if (!ctx->prof) return;
  hipEvent_t e0;
  if (hipEventCreate(&e0) != hipSuccess) return;
  if (hipEventCreate(e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    *e1 = nullptr;
    return;
  }
  (void)hipEventRecord(e0, st);  // a failed record shows up in fhe_profile_read
  a.ev.push_back({e0, *e1});
}
static void prof_end(fhe_ctx* ctx, ProfAcc& a, hipStream_t st, hipEvent_t e1, int64_t items) {
  if (!ctx->prof || !e1) return;
  (void)hipEventRecord(e1, st);
  a.launches += 1;
  a.items += items;
}

// the MFMA key switch's digit + body workspace of lane 0 or 1, grown to
// `count` ciphertexts (a grow synchronises the device: callers that run two
// lanes reserve both before launching on either)
static int ks_reserve(fhe_ctx* ctx, int64_t count, int lane) {
  const fhe_params& p = ctx->p;
  const int K = p.k * p.N * p.ks_level;
  const size_t need = (size_t)((count + 15) / 16) * 16 * K + 8 * (size_t)count;
  return reserve(ctx, ctx->ks_ws[lane], need, FHE_E_DEVICE, "hipMalloc of the key-switch workspace failed");
}

static int keyswitch_lane(fhe_ctx* ctx, const uint64_t* d_big, int64_t count, int32_t shift, uint64_t add_body,
                          uint64_t* d_small, hipStream_t st, int lane) {
  const fhe_params& p = ctx->p;
  const int64_t tiles = (count + KS_TC - 1) / KS_TC;
  if (tiles > 65535) return fail(ctx, FHE_E_ARG, "keyswitch batch too large: split the call");
  if (ctx->ks_variant == 2) {
    const int K = p.k * p.N * p.ks_level, KB = K / 64, n1 = p.n + 1, NB = ks_nb(p), CB = ks_cb(p);
    const int64_t ncb = (count + 15) / 16;
    const size_t dbytes = (size_t)ncb * 16 * K;
    int rc = ks_reserve(ctx, count, lane);
    if (rc) return rc;
    if (ncb > 65535) return fail(ctx, FHE_E_ARG, "keyswitch batch too large: split the call");
    void* ws = ctx->ks_ws[lane].p;
    uint32_t* D = (uint32_t*)ws;
    u64* body = (u64*)((char*)ws + dbytes);
    const int R = ks_round_bits(p);
    const int64_t ctb = (count + KSM_CTS - 1) / KSM_CTS, ktiles = ctb * (NB / CB);
    int force = 0;
#ifdef FHEICP_KS_AB  // A/B builds only: the split forced (tools/build_variant.sh)
    if (const char* e = getenv("FHEICP_KS_S")) force = std::max(1, atoi(e));
#endif
    const auto [S, kslice] = ksm_split(KB, ktiles, 512, force);
    hipEvent_t e1;
    prof_begin(ctx, ctx->prof_ks, st, &e1);
    // the digits kernel also zeroes the output the split's atomics add into
    hipLaunchKernelGGL(k_ks_digits, dim3((unsigned)(p.k * p.N / 64), (unsigned)ncb), dim3(256), 0, st, d_big, count,
                       p.k * p.N, p.ks_base_log, p.ks_level, shift, add_body, KB, D, body, S > 1 ? n1 : 0, d_small);
    const dim3 gks((unsigned)(ktiles * S));
    const bool known = ksm_dispatch(8 - R / 8, CB, [&, S = S, kslice = kslice](auto q, auto c) {
      static const std::string name = ksm_name("k_keyswitch_mfma", q, c);  // one per instantiation
      ctx->prof_ks.kernel = name.c_str();
      hipLaunchKernelGGL((k_keyswitch_mfma<q, c>), gks, dim3(256), 0, st, (const v4i*)D, (const v4i*)ctx->ksk8, body,
                         count, n1, NB, KB, R, S, kslice, d_small);
    });
    if (!known) return fail(ctx, FHE_E_ARG, "key-switch byte planes out of range");
    prof_end(ctx, ctx->prof_ks, st, e1, count);
    HIPCHK(ctx, hipGetLastError());
    return FHE_OK;
  }
  HIPCHK(ctx, hipMemsetAsync(d_small, 0, 8 * (size_t)count * (p.n + 1), st));
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_ks, st, &e1);
  ctx->prof_ks.kernel = "k_keyswitch";
  hipLaunchKernelGGL(k_keyswitch, dim3((p.n + 1 + 255) / 256, (unsigned)tiles, KS_SPLIT), dim3(256), 0, st, d_big,
                     count, p.k * p.N, p.n, p.ks_level, p.ks_base_log, shift, add_body, ctx->ksk, ctx->ksk_colsum,
                     ks_round_bits(p), d_small);
  prof_end(ctx, ctx->prof_ks, st, e1, count);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// The gadget key switches and the both-private product run that GEMM on 8
// unrounded byte planes, one column block per workgroup: rows x KB*64 digits
// `D` times the planes `K8` (KB*64 x NB*16), plus `body` on column n1 - 1,
// into the rows x n1 words of `M`. gemm81_split is its K split, which the
// caller's digits kernel needs first: with S > 1 that kernel zeroes M for the
// partial sums. gemm81 names the kernel in the caller's bucket and launches it
// between the caller's own kernels, inside the caller's prof_begin / prof_end.
static KsmSplit gemm81_split(int64_t rows, int NB, int KB) {
  return ksm_split(KB, (rows + KSM_CTS - 1) / KSM_CTS * NB, 512);
}
static int gemm81(fhe_ctx* ctx, ProfAcc& acc, const char* what, const void* D, const void* K8, const u64* body,
                  int64_t rows, int n1, int NB, int KB, u64* M, hipStream_t st) {
  const auto [S, kslice] = gemm81_split(rows, NB, KB);
  const int64_t grid = (rows + KSM_CTS - 1) / KSM_CTS * NB * S;
  // cannot fire below the callers' own limits (65,535 blocks of 16 rows; a
  // both-private workspace of 2^31 grid tiles is past any device's memory)
  if (grid > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, std::string(what) + " batch too large: split the call");
  acc.kernel = "k_keyswitch_mfma<8, 1>";
  hipLaunchKernelGGL((k_keyswitch_mfma<8, 1>), dim3((unsigned)grid), dim3(256), 0, st, (const v4i*)D, (const v4i*)K8,
                     body, rows, n1, NB, KB, 0, S, kslice, M);
  return FHE_OK;
}

// largest input shift whose key-switch tie coins (bits 62 - prec - j of the
// shifted input, j < ks_level) are all input bits, not the zeros shifted in
static int ks_max_shift(const fhe_params& p) { return 63 - p.ks_level * p.ks_base_log - p.ks_level; }
int fhe_keyswitch_batch(fhe_ctx* ctx, const uint64_t* d_big, int64_t count, int32_t shift, uint64_t add_body,
                        uint64_t* d_small, void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (count < 0 || shift < 0 || shift > ks_max_shift(ctx->p) || (count > 0 && (!d_big || !d_small)))
    return fail(ctx, FHE_E_ARG, "bad keyswitch arguments (shift must be in [0, 63 - ks_level * (ks_base_log + 1)])");
  if (count == 0) return FHE_OK;
  return keyswitch_lane(ctx, d_big, count, shift, add_body, d_small, (hipStream_t)stream, 0);
}

#ifdef FHEICP_AB
// A/B-only v4 shapes (FHEICP_V4_G = 1 or 2 for the 32-bit-accumulator
// kernels, FHEICP_V4_FL per-ciphertext hand-offs, FHEICP_V4_DBG timing
// experiments); false when the shipped dispatch applies.
static bool launch_br_ab(fhe_ctx* ctx, const fhe_params& p, const uint64_t* d_small, int64_t count, const BrTv& tv, int mode, uint64_t* out,
                         uint64_t* ct_v, uint64_t* refreshed, uint64_t* sign, const c64* bsk_fft, hipStream_t st,
                         const char** name) {
  const bool a32 = v4_a32(ctx, p);
#define AB4(L, A32, D, GG, FLAGS)                                                                               do {                                                                                                            hipLaunchKernelGGL((k_blind_rotate_v4<L, A32, D, GG, FLAGS>), dim3((unsigned)((count + GG - 1) / GG)),                           dim3(v4::nthreads(GG)), 0, st, d_small, count, p.n, p.pbs_base_log, bsk_fft,                               ctx->tw4, tv, mode, out, ct_v, refreshed, sign);                                           *name = "k_blind_rotate_v4<" #L ", " #A32 ", " #D ", " #GG ", " #FLAGS ", 0>";                                    return true;                                                                                                } while (0)
#define AB4G(L, A32, D, GG)   do { if (ctx->v4_fl && GG > 1) AB4(L, A32, D, GG, true); else AB4(L, A32, D, GG, false); } while (0)
#define AB4D(D)   do { if (ctx->v4_g == 1) AB4G(2, true, D, 1); else if (ctx->v4_g == 2) AB4G(2, true, D, 2); else AB4G(2, true, D, 4); } while (0)
  if (ctx->v4_dbg && p.pbs_level == 2 && a32) {
    switch (ctx->v4_dbg) {
      case 1: AB4D(1); case 2: AB4D(2); case 4: AB4D(4); case 8: AB4D(8); case 16: AB4D(16);
      case 32: AB4D(32); case 6: AB4D(6); case 128: AB4D(128); default: AB4D(63);
    }
  }
  if (ctx->v4s && a32) {  // FHEICP_V4S=1: key-stationary products for the 32-bit kernels too
    if (p.pbs_level == 1)
      hipLaunchKernelGGL((k_blind_rotate_v4s<1, true>), dim3((unsigned)((count + 3) / 4)), dim3(v4::nthreads(4)), 0,
                         st, d_small, count, p.n, p.pbs_base_log, bsk_fft, ctx->tw4, tv, mode, out, ct_v, refreshed, sign);
    else
      hipLaunchKernelGGL((k_blind_rotate_v4s<2, true>), dim3((unsigned)((count + 3) / 4)), dim3(v4::nthreads(4)), 0,
                         st, d_small, count, p.n, p.pbs_base_log, bsk_fft, ctx->tw4, tv, mode, out, ct_v, refreshed, sign);
    *name = "k_blind_rotate_v4s<A32>";
    return true;
  }
  // shapes other than the shipped ones; the 64-bit v4 kernels (v4s ships)
  if (!(ctx->v4_g == 1 || ctx->v4_fl || ctx->v4_g == 2)) return false;
  const int G = ctx->v4_g;
  switch (p.pbs_level) {
    case 1:
      if (a32) { if (G == 1) AB4G(1, true, 0, 1); else if (G == 2) AB4G(1, true, 0, 2); else AB4G(1, true, 0, 4); }
      else { if (G == 1) AB4G(1, false, 0, 1); else if (G == 2) AB4G(1, false, 0, 2); else AB4G(1, false, 0, 4); }
      break;
    case 2:
      if (a32) { if (G == 1) AB4G(2, true, 0, 1); else if (G == 2) AB4G(2, true, 0, 2); else AB4G(2, true, 0, 4); }
      else { if (G == 1) AB4G(2, false, 0, 1); else if (G == 2) AB4G(2, false, 0, 2); else AB4G(2, false, 0, 4); }
      break;
    case 3:
      if (G == 1) AB4G(3, false, 0, 1); else if (G == 2) AB4G(3, false, 0, 2); else AB4G(3, false, 0, 4);
      break;
  }
#undef AB4
#undef AB4G
#undef AB4D
  return false;
}
#endif

// gad = 1 / 2: the fast / fast2 gadget and its key (fhe_params.pbs_fast*_*),
// else the main one. The launched instantiation's name (as rocprofv3 prints
// it) is recorded in the profile bucket (fhe_profile_kernel_name).
static int launch_br(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, BrTv tv, int mode, uint64_t* out,
                     uint64_t* ct_v, uint64_t* refreshed, uint64_t* sign, hipStream_t st, int gad = 0) {
  const bool fast = gad > 0 && fast_level(ctx->p, gad);
  const fhe_params p = fast ? fast_params(ctx->p, gad) : ctx->p;
  const c64* bsk_fft = fast ? ctx->bskf_fft[gad - 1] : ctx->bsk_fft;
  const int var = variant_for(ctx, p);
  hipEvent_t e1;
  ProfAcc& prof = fast ? ctx->prof_brf[gad - 1] : ctx->prof_br;
  prof_begin(ctx, prof, st, &e1);
  const char* name = nullptr;
  const dim3 g((unsigned)count), b(64);
#define BR(LOGM, K)                                                                                           \
  do {                                                                                                        \
    hipLaunchKernelGGL((k_blind_rotate<LOGM, K>), g, b, 0, st, d_small, p.n, p.pbs_level, p.pbs_base_log,    \
                       bsk_fft, ctx->tw, ctx->twist, tv, mode, out, ct_v, refreshed, sign);                  \
    name = "k_blind_rotate<" #LOGM ", " #K ", BrTv>";                                                         \
  } while (0)
#define BRV(V, K, W)                                                                                          \
  do {                                                                                                        \
    hipLaunchKernelGGL((k_blind_rotate_mw<V, K, W>), g, dim3(V::NT), 0, st, d_small, p.n, p.pbs_level,        \
                       p.pbs_base_log, bsk_fft, ctx->tw, ctx->twist, tv, mode, out, ct_v, refreshed, sign);   \
    name = "k_blind_rotate_mw<fhei::" #V ", " #K ", " #W ", BrTv>";                                           \
  } while (0)
#define BR4F(L, A32, D, GG, FLAGS, B)                                                                         \
  do {                                                                                                        \
    hipLaunchKernelGGL((k_blind_rotate_v4<L, A32, D, GG, FLAGS, B>), dim3((unsigned)((count + GG - 1) / GG)), \
                       dim3(v4::nthreads(GG)), 0, st, d_small, count, p.n, p.pbs_base_log, bsk_fft, ctx->tw4, \
                       tv, mode, out, ct_v, refreshed, sign);                                                 \
    name = "k_blind_rotate_v4<" #L ", " #A32 ", " #D ", " #GG ", " #FLAGS ", " #B ">";                         \
  } while (0)
  // The shipped N = 1024, k = 2 instances: the multi-bit kernels for fast
  // gadgets with pbs_fast*_group = 2; v4 at 4 ciphertexts per workgroup (3
  // waves per SIMD, <= 168 VGPRs) for the 32-bit accumulators; v4s for the
  // 64-bit ones. Other shapes are A/B builds (FHEICP_AB).
  bool done = false;
#ifdef FHEICP_AB
  if (p.N == 1024 && p.k == 2 && var == 4) done = launch_br_ab(ctx, p, d_small, count, tv, mode, out, ct_v, refreshed, sign,
                                                               bsk_fft, st, &name);
#endif
  if (done) {
  } else if (fast && mb_for(ctx->p, gad)) {
    // multi-bit rotation, key-stationary products (k_blind_rotate_mb)
    const dim3 gm((unsigned)((count + 3) / 4)), bm(v4::nthreads(4));
#define MBD(L, D, B)                                                                                            \
  hipLaunchKernelGGL((k_blind_rotate_mb<L, D, B>), gm, bm, 0, st, d_small, count, p.n, p.pbs_base_log, bsk_fft, \
                     ctx->tw4, ctx->psi, tv, mode, out, ct_v, refreshed, sign)
#ifdef FHEICP_AB
    if (ctx->mb_dbg) {
      const int w = ctx->mb_dbg >> 8;
      if (ctx->mb_dbg == 2) { if (p.pbs_level == 1) MBD(1, 2, 0); else MBD(2, 2, 0); }
      else if (ctx->mb_dbg == 16) { if (p.pbs_level == 1) MBD(1, 16, 0); else MBD(2, 16, 0); }
      else if (ctx->mb_dbg == 32) { if (p.pbs_level == 1) MBD(1, 32, 0); else MBD(2, 32, 0); }
      else if (ctx->mb_dbg == 48) { if (p.pbs_level == 1) MBD(1, 48, 0); else MBD(2, 48, 0); }
      else if (ctx->mb_dbg == 64) { if (p.pbs_level == 1) MBD(1, 64, 0); else MBD(2, 64, 0); }
      else if (ctx->mb_dbg == 18) { if (p.pbs_level == 1) MBD(1, 18, 0); else MBD(2, 18, 0); }
      else if (ctx->mb_dbg == 130) { if (p.pbs_level == 1) MBD(1, 130, 0); else MBD(2, 130, 0); }
      else if (w == 0) { if (p.pbs_level == 1) MBD(1, 128, 0); else MBD(2, 128, 0); }
      else if (w == 1) { if (p.pbs_level == 1) MBD(1, 128 + 256, 0); else MBD(2, 128 + 256, 0); }
      else { if (p.pbs_level == 1) MBD(1, 128 + 512, 0); else MBD(2, 128 + 512, 0); }
      name = "k_blind_rotate_mb<DBG>";
    } else
#endif
    // wide (48-bit) accumulators (L * beta > 31 or L > 2): the deep gadgets
    if (!(p.pbs_level <= 2 && p.pbs_level * p.pbs_base_log <= 31)) {
#define MB64(L)                                                                                                  \
  hipLaunchKernelGGL((k_blind_rotate_mb64<L, 0>), gm, bm, 0, st, d_small, count, p.n, p.pbs_base_log, bsk_fft,   \
                     ctx->tw4, ctx->psi, tv, mode, out, ct_v, refreshed, sign);                                 \
  name = "k_blind_rotate_mb64<" #L ", 0, BrTv>"
      switch (p.pbs_level) {
        case 1: MB64(1); break;
        case 2: MB64(2); break;
        case 3: MB64(3); break;
        case 4: MB64(4); break;
        case 5: MB64(5); break;
        case 6: MB64(6); break;
        case 7: MB64(7); break;
        case 8: MB64(8); break;
        default: return fail(ctx, FHE_E_ARG, "multi-bit blind rotation: pbs_level > 8");
      }
#undef MB64
    } else
    // the shipped fast gadgets (23,1) and (15,2) with their base log fixed
    if (p.pbs_level == 1 && p.pbs_base_log == 23) {
      MBD(1, 0, 23);
      name = "k_blind_rotate_mb<1, 0, 23, BrTv>";
    } else if (p.pbs_level == 1) {
      MBD(1, 0, 0);
      name = "k_blind_rotate_mb<1, 0, 0, BrTv>";
    } else if (p.pbs_base_log == 15) {
      MBD(2, 0, 15);
      name = "k_blind_rotate_mb<2, 0, 15, BrTv>";
    } else {
      MBD(2, 0, 0);
      name = "k_blind_rotate_mb<2, 0, 0, BrTv>";
    }
#undef MBD
  } else if (p.N == 1024 && p.k == 2 && var == 4 && !v4_a32(ctx, p)) {
    // 64-bit accumulators: the key-stationary v4s kernels, 4 ciphertexts per
    // workgroup (15.9 vs 20.7 ms per 1024 at (12,3) for v4 at 2 per workgroup)
#define BR4S(L, B)                                                                                            \
  do {                                                                                                        \
    hipLaunchKernelGGL((k_blind_rotate_v4s<L, false, 0, B>), dim3((unsigned)((count + 3) / 4)),              \
                       dim3(v4::nthreads(4)), 0, st, d_small, count, p.n, p.pbs_base_log, bsk_fft, ctx->tw4,  \
                       tv, mode, out, ct_v, refreshed, sign);                                                 \
    name = "k_blind_rotate_v4s<" #L ", false, 0, " #B ">";                                                     \
  } while (0)
    // run-time base log: fixing (12, 3)'s at compile time made the compiler
    // emit 144 more f64 instructions per step and a 56-byte spill
    switch (p.pbs_level) {
      case 1: BR4S(1, 0); break;
      case 2: BR4S(2, 0); break;
      case 3: BR4S(3, 0); break;
      // the deep gadgets (C5's main and mid ones): 1.5-1.6x faster than v2,
      // e.g. (6,7) 29.5 vs 46.7 ms and (8,5) 23.0 vs 35.1 ms per 1024
      case 4: BR4S(4, 0); break;
      case 5: BR4S(5, 0); break;
      case 6: BR4S(6, 0); break;
      case 7: BR4S(7, 0); break;
      case 8: BR4S(8, 0); break;
      default: return fail(ctx, FHE_E_ARG, "v4s blind rotation: pbs_level > 8");
    }
#undef BR4S
  } else if (p.N == 1024 && p.k == 2 && var == 4) {
    switch (p.pbs_level) {
      // (23, 1) and (15, 2), the classic gadgets of the parameter table, with
      // their base log fixed; others on the run-time instances
      case 1:
        if (p.pbs_base_log == 23) BR4F(1, true, 0, 4, false, 23);
        else BR4F(1, true, 0, 4, false, 0);
        break;
      case 2:
        if (p.pbs_base_log == 15) BR4F(2, true, 0, 4, false, 15);
        else BR4F(2, true, 0, 4, false, 0);
        break;
      default: return fail(ctx, FHE_E_ARG, "v4 blind rotation: 32-bit accumulators need pbs_level <= 2");
    }
  } else if (p.N == 256 && p.k == 1) BR(7, 1);
  else if (p.N == 256 && p.k == 2) BR(7, 2);
  else if (p.N == 512 && p.k == 1) BR(8, 1);
  else if (p.N == 512 && p.k == 2) BR(8, 2);
  else if (p.N == 1024 && p.k == 1) BRV(V2, 1, 2);
  else if (p.N == 1024 && p.k == 2) BRV(V2, 2, 2);
  else if (p.N == 2048 && p.k == 1) BR(10, 1);
  else return fail(ctx, FHE_E_ARG, "unsupported (N, k)");
#undef BR
#undef BR4F
#undef BRV
  prof.kernel = name;
  prof_end(ctx, prof, st, e1, count);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_pbs_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, uint64_t tv, uint64_t* d_out, void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!d_small || !d_out))) return fail(ctx, FHE_E_ARG, "bad pbs arguments");
  if (count == 0) return FHE_OK;
  return launch_br(ctx, d_small, count, BrTv{tv, 0, 0}, 0, d_out, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int fhe_pbs_gadget_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, int32_t gadget, uint64_t tv,
                         uint64_t* d_out, void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (count < 0 || gadget < 0 || gadget >= NGAD || (count > 0 && (!d_small || !d_out)))
    return fail(ctx, FHE_E_ARG, "bad pbs-gadget arguments");
  if (gadget > 0 && !fast_level(ctx->p, gadget)) return fail(ctx, FHE_E_STATE, "no such fast gadget in these parameters");
  if (count == 0) return FHE_OK;
  return launch_br(ctx, d_small, count, BrTv{tv, 0, 0}, 0, d_out, nullptr, nullptr, nullptr, (hipStream_t)stream,
                   gadget);
}

static int log2i(int x) {
  int l = 0;
  while ((1 << l) < x) ++l;
  return l;
}

int fhe_pbs_lut_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, uint64_t base, uint64_t step,
                      int32_t log_slots, uint64_t* d_out, void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  const int logN = log2i(ctx->p.N);
  if (count < 0 || (count > 0 && (!d_small || !d_out)) || log_slots < 0 || log_slots > logN)
    return fail(ctx, FHE_E_ARG, "bad pbs-lut arguments");
  if (count == 0) return FHE_OK;
  return launch_br(ctx, d_small, count, BrTv{base, step, logN - log_slots}, 0, d_out, nullptr, nullptr, nullptr,
                   (hipStream_t)stream);
}

// The gadget fhe_pbs_table_batch runs on: the most precise (smallest
// bootstrap variance) multi-bit gadget of the set, whose rotation is the
// shipped k_blind_rotate_mb / _mb64 family (e.g. (15,2) at P = 16, (5,8) at
// P = 26); 0 (the classic main gadget, v2 / v1 kernels) when the set has none.
static int table_gadget(const fhe_params& p) {
  int best = 0;
  double v = 0;
  for (int g = 1; g < NGAD; ++g) {
    if (!mb_for(p, g)) continue;
    const double vg = pbs_var(p, gadget_base_log(p, g), gadget_level(p, g), 2);
    if (!best || vg < v) best = g, v = vg;
  }
  return best;
}

// The table bootstrap on a multi-bit gadget: the sign extraction's kernels
// (k_blind_rotate_mb: 32-bit accumulators, (23,1) and (15,2) with their base
// log fixed as there; k_blind_rotate_mb64: 48-bit, levels 2-8) instantiated
// for the table test vector (BrTvLut), with that gadget's multi-bit key.
static int launch_br_table_mb(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, const BrTvLut& tv, uint64_t* out,
                              hipStream_t st, int gad) {
  const fhe_params q = fast_params(ctx->p, gad);
  const c64* bsk = ctx->bskf_fft[gad - 1];
  ProfAcc& prof = ctx->prof_brf[gad - 1];
  hipEvent_t e1;
  prof_begin(ctx, prof, st, &e1);
  const char* name = nullptr;
  const dim3 gm((unsigned)((count + 3) / 4)), bm(v4::nthreads(4));
#define MBT(L, B)                                                                                                  \
  do {                                                                                                             \
    hipLaunchKernelGGL((k_blind_rotate_mb<L, 0, B, BrTvLut>), gm, bm, 0, st, d_small, count, q.n, q.pbs_base_log,   \
                       bsk, ctx->tw4, ctx->psi, tv, 0, out, nullptr, nullptr, nullptr);                            \
    name = "k_blind_rotate_mb<" #L ", 0, " #B ", BrTvLut>";                                                        \
  } while (0)
#define MB64T(L)                                                                                                   \
  do {                                                                                                             \
    hipLaunchKernelGGL((k_blind_rotate_mb64<L, 0, BrTvLut>), gm, bm, 0, st, d_small, count, q.n, q.pbs_base_log,    \
                       bsk, ctx->tw4, ctx->psi, tv, 0, out, nullptr, nullptr, nullptr);                            \
    name = "k_blind_rotate_mb64<" #L ", 0, BrTvLut>";                                                              \
  } while (0)
  if (q.pbs_level <= 2 && q.pbs_level * q.pbs_base_log <= 31) {
    if (q.pbs_level == 1) {
      if (q.pbs_base_log == 23) MBT(1, 23);
      else MBT(1, 0);
    } else {
      if (q.pbs_base_log == 15) MBT(2, 15);
      else MBT(2, 0);
    }
  } else {
    switch (q.pbs_level) {
      case 2: MB64T(2); break;
      case 3: MB64T(3); break;
      case 4: MB64T(4); break;
      case 5: MB64T(5); break;
      case 6: MB64T(6); break;
      case 7: MB64T(7); break;
      case 8: MB64T(8); break;
      default: return fail(ctx, FHE_E_ARG, "table bootstrap: no multi-bit kernel for this gadget level");
    }
  }
#undef MBT
#undef MB64T
  prof.kernel = name;
  prof_end(ctx, prof, st, e1, count);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// The table bootstrap on the classic main gadget (parameter sets without a
// multi-bit gadget): the v2 kernel at N = 1024 (v1 otherwise), instantiated
// for the wide test-vector argument (BrTvLut); the compare's hot kernels keep
// the three-word one.
static int launch_br_table(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, const BrTvLut& tv, uint64_t* out,
                           hipStream_t st) {
  const fhe_params& p = ctx->p;
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_br, st, &e1);
  const char* name = nullptr;
  const dim3 g((unsigned)count), b(64);
#define BRT(LOGM, K)                                                                                          \
  do {                                                                                                        \
    hipLaunchKernelGGL((k_blind_rotate<LOGM, K, BrTvLut>), g, b, 0, st, d_small, p.n, p.pbs_level,            \
                       p.pbs_base_log, ctx->bsk_fft, ctx->tw, ctx->twist, tv, 0, out, nullptr, nullptr, nullptr); \
    name = "k_blind_rotate<" #LOGM ", " #K ", BrTvLut>";                                                      \
  } while (0)
  if (p.N == 1024 && variant_for(ctx, p) == 4) {
    // the BSK is in the v4 FFT layout: build a v2-layout copy once
    if (!ctx->bsk_fft_v2) {
      HIPCHK(ctx, hipMalloc(&ctx->bsk_fft_v2, sizeof(c64) * fhe_bsk_words(&p) / 2));
      const int npoly = (int)(fhe_bsk_words(&p) / p.N);
      hipLaunchKernelGGL(k_bsk_to_fft_mw<V2>, dim3(npoly), dim3(V2::NT), 0, st, ctx->bsk, npoly, ctx->tw, ctx->twist,
                         ctx->bsk_fft_v2);
      // once per key: a later table bootstrap on another stream must not
      // read the copy before this conversion has finished
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipStreamSynchronize(st));
    }
  }
  const c64* bsk = (p.N == 1024 && ctx->bsk_fft_v2) ? ctx->bsk_fft_v2 : ctx->bsk_fft;
  if (p.N == 1024) {
    if (p.k == 1) {
      hipLaunchKernelGGL((k_blind_rotate_mw<V2, 1, 2, BrTvLut>), g, dim3(V2::NT), 0, st, d_small, p.n, p.pbs_level,
                         p.pbs_base_log, bsk, ctx->tw, ctx->twist, tv, 0, out, nullptr, nullptr, nullptr);
      name = "k_blind_rotate_mw<fhei::V2, 1, 2, BrTvLut>";
    } else {
      hipLaunchKernelGGL((k_blind_rotate_mw<V2, 2, 2, BrTvLut>), g, dim3(V2::NT), 0, st, d_small, p.n, p.pbs_level,
                         p.pbs_base_log, bsk, ctx->tw, ctx->twist, tv, 0, out, nullptr, nullptr, nullptr);
      name = "k_blind_rotate_mw<fhei::V2, 2, 2, BrTvLut>";
    }
  } else if (p.N == 256 && p.k == 1) BRT(7, 1);
  else if (p.N == 256 && p.k == 2) BRT(7, 2);
  else if (p.N == 512 && p.k == 1) BRT(8, 1);
  else if (p.N == 512 && p.k == 2) BRT(8, 2);
  else if (p.N == 2048 && p.k == 1) BRT(10, 1);
  else return fail(ctx, FHE_E_ARG, "unsupported (N, k)");
#undef BRT
  ctx->prof_br.kernel = name;
  prof_end(ctx, ctx->prof_br, st, e1, count);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_pbs_table_gadget_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, int32_t gadget,
                               const int64_t* d_lut, int32_t lut_bits, uint64_t* d_out, void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  const int logN = log2i(ctx->p.N);
  if (count < 0 || lut_bits < 0 || lut_bits > logN - 1 || !d_lut || (count > 0 && (!d_small || !d_out)))
    return fail(ctx, FHE_E_ARG, "bad pbs-table arguments (0 <= lut_bits <= log2(N) - 1)");
  if (gadget < 0 || gadget >= NGAD || (gadget > 0 && !mb_for(ctx->p, gadget)))
    return fail(ctx, FHE_E_ARG, "pbs-table gadget must be 0 (the classic main gadget) or a multi-bit gadget of "
                                "these parameters");
  if (count == 0) return FHE_OK;
  BrTvLut tv{0, 0, 0, logN - lut_bits, 1 << lut_bits, d_lut, 1ull << (64 - ctx->p.msg_bits)};
  if (gadget > 0) return launch_br_table_mb(ctx, d_small, count, tv, d_out, (hipStream_t)stream, gadget);
  return launch_br_table(ctx, d_small, count, tv, d_out, (hipStream_t)stream);
}

int fhe_pbs_table_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, const int64_t* d_lut, int32_t lut_bits,
                        uint64_t* d_out, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  return fhe_pbs_table_gadget_batch(ctx, d_small, count, table_gadget(ctx->p), d_lut, lut_bits, d_out, stream);
}

int fhe_pbs_table_gadget(const fhe_params* params) {
  std::string why;
  if (validate(params, why)) return FHE_E_ARG;
  return table_gadget(*params);
}

static int ensure_ws(fhe_ctx* ctx, size_t bytes) {
  return reserve(ctx, ctx->ws, bytes, FHE_E_DEVICE, "hipMalloc of the context workspace failed");
}

// bit extraction driver; `small` is caller-provided scratch (count x (n+1))
static int bit_extract(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_ref, uint64_t* d_sign,
                       uint64_t* small, hipStream_t st) {
  const fhe_params& p = ctx->p;
  const int P = p.msg_bits;
  HIPCHK(ctx, hipMemsetAsync(d_ref, 0, 8 * (size_t)count * fhe_big_lwe_words(&p), st));
  for (int i = 0; i < P; ++i) {
    int rc = fhe_keyswitch_batch(ctx, d_ct_v, count, P - 1 - i, 1ull << 62, small, st);
    if (rc) return rc;
    rc = launch_br(ctx, small, count, BrTv{1ull << (63 - P + i), 0, 0}, 1, nullptr, d_ct_v, d_ref,
                   (i == P - 1) ? d_sign : nullptr, st);
    if (rc) return rc;
  }
  return FHE_OK;
}

// Sign of the msg_bits-bit value v in d_ct_v (consumed) with d-bit digits
// (DESIGN.md §3.4): the low m = P - d bits are cleared LSB-first, each full
// digit [b, b+c) by two bootstraps (its top bit by a sign bootstrap; then,
// with a zero padding bit, its c-1 low bits by a 2^(c-1)-slot staircase LUT),
// a leftover of 1-2 bits by single-bit rounds; the sign of the top d bits is
// the sign of v.
int fhe_sign_digit_bits(const fhe_params* params) {
  std::string why;
  if (validate(params, why)) return -1;
  return sign_digits(*params);
}

int fhe_sign_pbs_count(const fhe_params* params) {
  std::string why;
  if (validate(params, why)) return -1;
  const int P = params->msg_bits, d = sign_digits(*params);
  if (P < 4) return P;
  const int m = P - d, r = m % d;
  return 2 * (m / d) + (r >= 3 ? 2 : r) + 1;
}

int fhe_sign_precise_rounds(const fhe_params* params) {
  std::string why;
  if (validate(params, why)) return -1;
  int d, j1, j2;
  sign_plan(*params, &d, &j1, &j2);
  return j1;
}

int fhe_sign_schedule(const fhe_params* params, int32_t* gadgets, int32_t cap) {
  std::string why;
  if (validate(params, why)) return FHE_E_ARG;
  int d, sched[64];
  const int R = sign_schedule(*params, &d, sched);
  for (int r = 0; r < R && r < cap; ++r)
    if (gadgets) gadgets[r] = sched[r];
  return R;
}

int fhe_sign_plan(const fhe_params* params, int32_t* digit_bits, int32_t* main_rounds, int32_t* fast_end) {
  std::string why;
  if (validate(params, why)) return FHE_E_ARG;
  int d, j1, j2;
  sign_plan(*params, &d, &j1, &j2);
  if (digit_bits) *digit_bits = d;
  if (main_rounds) *main_rounds = j1;
  if (fast_end) *fast_end = j2;
  return FHE_OK;
}

// Trace of a sign extraction (fhe_sign_trace_batch, measurement only): an
// explicit gadget per round instead of sign_schedule's, a stop after the
// first `rounds` bootstraps, and the rotation exponent of every round's input
// (k_ms_phase) into phase[round * count + c].
struct SignTrace {
  const int* sched = nullptr;
  int rounds = 0;
  uint32_t* phase = nullptr;
};

extern "C++" {
template <class Step>
static int sign_walk(const fhe_params& p, int d, Step&& step, uint64_t* d_sign);
}

static int sign_extract(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_sign, uint64_t* small,
                        hipStream_t st, int lane = 0, const SignTrace* tr = nullptr) {
  const fhe_params& p = ctx->p;
  const int P = p.msg_bits, logN = log2i(p.N);
  int d = 0, sched[64];
  if (P < 4) {
    for (int r = 0; r < P; ++r) sched[r] = 0;
  } else {
    sign_schedule(p, &d, sched);
  }
  if (tr && tr->sched) {
    int dd, tmp[64];
    const int R = P < 4 ? P : sign_schedule(p, &dd, tmp);
    for (int r = 0; r < R; ++r) sched[r] = tr->sched[r];
  }
  int round = 0;  // bootstraps issued so far; round r runs on gadget sched[r]
  // one round: key switch of v << shift, centred by `add`, then the bootstrap
  auto step = [&](int shift, uint64_t add, BrTv tv, int mode, uint64_t* sign) -> int {
    if (tr && tr->rounds && round >= tr->rounds) return FHE_OK;
    int r = keyswitch_lane(ctx, d_ct_v, count, shift, add, small, st, lane);
    if (r) return r;
    if (tr && tr->phase) {
      hipLaunchKernelGGL(k_ms_phase, dim3((unsigned)count), dim3(64), 0, st, p.n, logN + 1,
                         gadget_group(p, sched[round]), ctx->s_small, small, count,
                         tr->phase + (size_t)round * count);
      HIPCHK(ctx, hipGetLastError());
    }
    return launch_br(ctx, small, count, tv, mode, nullptr, d_ct_v, nullptr, sign, st, sched[round++]);
  };
  return sign_walk(p, d, step, d_sign);
}

// The rounds of a sign extraction in order (shifts, centring constants and
// test vectors), each handed to step(shift, add, tv, mode, sign): shared by
// sign_extract and the group form (fhe_sign_group_batch)
extern "C++" {
template <class Step>
static int sign_walk(const fhe_params& p, int d, Step&& step, uint64_t* d_sign) {
  const int P = p.msg_bits, logN = log2i(p.N);
  int rc;
  if (P < 4) {
    for (int i = 0; i < P; ++i)
      if ((rc = step(P - 1 - i, 1ull << 62, BrTv{1ull << (63 - P + i), 0, 0}, 1, (i == P - 1) ? d_sign : nullptr)))
        return rc;
    return FHE_OK;
  }
  const int m = P - d;
  // one c-bit digit at bit b: the pair of rounds on v << (P-b-c) centred by 2^(63-c)
  auto digit = [&](int b, int c) -> int {
    int r;
    // digit MSB (bit b+c-1): sign bootstrap, ct_v -= [bit] * 2^(b+c-1) * Delta
    if ((r = step(P - b - c, 1ull << (63 - c), BrTv{1ull << (62 - P + b + c), 0, 0}, 1, nullptr))) return r;
    // bits [b, b+c-1): top bit is now 0 -> 2^(c-1)-slot staircase, output D' * 2^b * Delta
    return step(P - b - c, 1ull << (63 - c), BrTv{0, 1ull << (64 - P + b), logN - (c - 1)}, 2, nullptr);
  };
  int b = 0;
  for (; b + d <= m; b += d)
    if ((rc = digit(b, d))) return rc;
  if (m - b >= 3) {
    if ((rc = digit(b, m - b))) return rc;
    b = m;
  }
  for (; b < m; ++b)
    if ((rc = step(P - b - 1, 1ull << 62, BrTv{1ull << (63 - P + b), 0, 0}, 1, nullptr))) return rc;
  // sign = MSB of the top digit [P-d, P)
  return step(0, 1ull << (63 - d), BrTv{1ull << 62, 0, 0}, 1, d_sign);
}
}  // extern "C++"

// The sign extraction of a large batch (>= PIPE_MIN ciphertexts) in two
// halves on two streams: each half runs its key switches and bootstraps in
// order, and the GPU overlaps one half's key switches and kernel tails with
// the other half's bootstraps. Below PIPE_MIN (one or two waves of
// workgroups) it stays on the caller's stream, so single-launch timings keep
// their meaning. FHEICP_PIPE=0 turns it off (A/B runs).
constexpr int64_t PIPE_MIN = 2048;
static int sign_extract_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_sign, uint64_t* small,
                              hipStream_t st) {
  static const bool off = [] {
    const char* e = getenv("FHEICP_PIPE");
    return e && atoi(e) == 0;
  }();
  static const int64_t pipe_min = [] {  // FHEICP_PIPE_MIN: A/B runs of the threshold
    const char* e = getenv("FHEICP_PIPE_MIN");
    return e ? (int64_t)std::max(8, atoi(e)) : PIPE_MIN;
  }();
  if (count < pipe_min || off) return sign_extract(ctx, d_ct_v, count, d_sign, small, st, 0);
  const fhe_params& p = ctx->p;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
  // the first half a whole number of 1024-ciphertext waves (256 four-ciphertext
  // workgroups, one per CU) nearest count / 2, so only the second half ends on
  // a partial wave: at 12,500 (a C4 shard) 6144 + 6356 runs 13 rounds of
  // workgroups where 6252 + 6248 ran 14 (6.1 waves each)
  const int64_t c0 = count < 2048 ? ((count / 2) + 3) & ~(int64_t)3
                                  : std::min(std::max((int64_t)1024, 1024 * ((count + 1024) / 2048)), count - 4),
                c1 = count - c0;
  for (int l = 0; l < 2; ++l)
    if (!ctx->lane_st[l]) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->lane_st[l], hipStreamNonBlocking));
  for (int l = 0; l < 3; ++l)
    if (!ctx->lane_ev[l]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->lane_ev[l], hipEventDisableTiming));
  // the MFMA key switch's per-lane workspaces (the VALU variant needs none)
  int rc = ctx->ks_variant == 2 ? ks_reserve(ctx, c0, 0) : FHE_OK;
  if (!rc && ctx->ks_variant == 2) rc = ks_reserve(ctx, c1, 1);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->lane_ev[0], st));
  for (int l = 0; l < 2; ++l) HIPCHK(ctx, hipStreamWaitEvent(ctx->lane_st[l], ctx->lane_ev[0], 0));
  rc = sign_extract(ctx, d_ct_v, c0, d_sign, small, ctx->lane_st[0], 0);
  if (!rc)
    rc = sign_extract(ctx, d_ct_v + (size_t)c0 * Wb, c1, d_sign + (size_t)c0 * Wb, small + (size_t)c0 * Ws,
                      ctx->lane_st[1], 1);
  // the caller's stream waits for both halves (also on an error, so nothing
  // queued on it can overtake work already launched on the lanes)
  for (int l = 0; l < 2; ++l) {
    HIPCHK(ctx, hipEventRecord(ctx->lane_ev[1 + l], ctx->lane_st[l]));
    HIPCHK(ctx, hipStreamWaitEvent(st, ctx->lane_ev[1 + l], 0));
  }
  return rc;
}

int fhe_sign_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_sign, void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!d_ct_v || !d_sign))) return fail(ctx, FHE_E_ARG, "bad sign arguments");
  if (count == 0) return FHE_OK;
  rc = ensure_ws(ctx, 8 * (size_t)count * fhe_small_lwe_words(&ctx->p));
  if (rc) return rc;
  return sign_extract_batch(ctx, d_ct_v, count, d_sign, (uint64_t*)ctx->ws.p, (hipStream_t)stream);
}

int fhe_sign_trace_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, const int32_t* h_sched, int32_t rounds,
                         uint64_t* d_sign, uint32_t* d_phase, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  const fhe_params& p = ctx->p;
  int d, tmp[64];
  const int R = p.msg_bits < 4 ? p.msg_bits : sign_schedule(p, &d, tmp);
  if (count < 0 || rounds < 0 || rounds > R || (count > 0 && !d_ct_v) ||
      (count > 0 && (rounds == 0 || rounds == R) && !d_sign))
    return fail(ctx, FHE_E_ARG, "bad sign-trace arguments (0 <= rounds <= the plan's bootstraps; d_sign when the "
                                "last round runs)");
  int sched[64];
  if (h_sched) {
    for (int r = 0; r < R; ++r) {
      const int g = h_sched[r];
      if (g < 0 || g >= NGAD || (g > 0 && !fast_level(p, g)))
        return fail(ctx, FHE_E_ARG, "sign-trace schedule names a gadget these parameters do not have");
      sched[r] = g;
    }
  }
  if (count == 0) return FHE_OK;
  rc = ensure_ws(ctx, 8 * (size_t)count * fhe_small_lwe_words(&p));
  if (rc) return rc;
  SignTrace tr;
  tr.sched = h_sched ? sched : nullptr;
  tr.rounds = rounds;
  tr.phase = d_phase;
  return sign_extract(ctx, d_ct_v, count, d_sign, (uint64_t*)ctx->ws.p, (hipStream_t)stream, 0, &tr);
}

int fhe_bit_extract_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_refreshed, uint64_t* d_sign,
                          void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!d_ct_v || !d_refreshed || !d_sign)))
    return fail(ctx, FHE_E_ARG, "bad bit-extract arguments");
  if (count == 0) return FHE_OK;
  rc = ensure_ws(ctx, 8 * (size_t)count * fhe_small_lwe_words(&ctx->p));
  if (rc) return rc;
  return bit_extract(ctx, d_ct_v, count, d_refreshed, d_sign, (uint64_t*)ctx->ws.p, (hipStream_t)stream);
}

static int compare_impl(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                        int64_t T, const ChaKey& K, uint64_t id0, int64_t* d_acc, int64_t* d_below, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_qx || !d_w || !d_acc || !d_below)))
    return fail(ctx, FHE_E_ARG, "bad compare arguments");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
  // workspace: ct_v (B big) | sign (B big) | small (B) | v (B); the B x D
  // input ciphertexts are never materialised (k_encrypt_linear)
  const size_t bytes = 8 * (2 * (size_t)B * Wb + (size_t)B * Ws + (size_t)B);
  rc = ensure_ws(ctx, bytes);
  if (rc) return rc;
  u64* ctv = (u64*)ctx->ws.p;
  u64* sgn = ctv + (size_t)B * Wb;
  u64* small = sgn + (size_t)B * Wb;
  int64_t* v = (int64_t*)(small + (size_t)B * Ws);
  rc = encrypt_linear_impl(ctx, d_qx, B, D, K, id0, d_w, cst - T, ctv, stream);
  if (rc) return rc;
  // The score comes from the leveled accumulator ciphertext (noise ~2^20,
  // as in the reference's leveled Concrete circuit); the PBS chain then
  // computes the encrypted threshold bit [acc < T] exactly.
  rc = fhe_decrypt_batch(ctx, ctv, B, v, stream);
  if (rc) return rc;
  rc = sign_extract_batch(ctx, ctv, B, sgn, small, st);
  if (rc) return rc;
  rc = fhe_decrypt_bits_batch(ctx, sgn, B, d_below, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_add_scalar, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, v, B, T, d_acc);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_compare_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                      int64_t T, uint64_t enc_seed, uint64_t id0, int64_t* d_acc, int64_t* d_below, void* stream) {
  return compare_impl(ctx, d_qx, B, D, d_w, cst, T, key_from_seed(enc_seed), id0, d_acc, d_below, stream);
}
int fhe_compare_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                          int64_t T, const uint32_t h_enc_key[8], uint64_t id0, int64_t* d_acc, int64_t* d_below,
                          void* stream) {
  ChaKey K;
  if (!key_arg(h_enc_key, K)) return fail(ctx, FHE_E_ARG, "null encryption key");
  return compare_impl(ctx, d_qx, B, D, d_w, cst, T, K, id0, d_acc, d_below, stream);
}

// The reference's own encrypted predict (fhe_similarity.py:142-160): the
// leveled circuit only. No key switch and no bootstrap; T only centres the
// accumulator in the msg_bits-bit encoding (acc - T must fit it).
static int score_impl(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                      int64_t T, const ChaKey& K, uint64_t id0, int64_t* d_acc, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_qx || !d_w || !d_acc))) return fail(ctx, FHE_E_ARG, "bad score arguments");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const size_t Wb = fhe_big_lwe_words(&p);
  // workspace: ct_v (B big) | v (B)
  rc = ensure_ws(ctx, 8 * ((size_t)B * Wb + (size_t)B));
  if (rc) return rc;
  u64* ctv = (u64*)ctx->ws.p;
  int64_t* v = (int64_t*)(ctv + (size_t)B * Wb);
  rc = encrypt_linear_impl(ctx, d_qx, B, D, K, id0, d_w, cst - T, ctv, stream);
  if (rc) return rc;
  rc = fhe_decrypt_batch(ctx, ctv, B, v, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_add_scalar, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, v, B, T, d_acc);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_score_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                    int64_t T, uint64_t enc_seed, uint64_t id0, int64_t* d_acc, void* stream) {
  return score_impl(ctx, d_qx, B, D, d_w, cst, T, key_from_seed(enc_seed), id0, d_acc, stream);
}
int fhe_score_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                        int64_t T, const uint32_t h_enc_key[8], uint64_t id0, int64_t* d_acc, void* stream) {
  ChaKey K;
  if (!key_arg(h_enc_key, K)) return fail(ctx, FHE_E_ARG, "null encryption key");
  return score_impl(ctx, d_qx, B, D, d_w, cst, T, K, id0, d_acc, stream);
}

int fhe_compare_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                             const uint32_t h_mask_key[8], const int64_t* d_w, int64_t cst, int64_t T,
                             int64_t* d_acc, int64_t* d_below, void* stream) {
  int rc = need_secret(ctx);
  if (rc) return rc;
  if ((rc = seeded_args(ctx, B, D, d_body, d_id0, d_w))) return rc;
  if (!h_mask_key || (B > 0 && (!d_acc || !d_below))) return fail(ctx, FHE_E_ARG, "bad seeded compare arguments");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
  // workspace: ct_v (B big) | sign (B big) | small (B) | v (B)
  rc = ensure_ws(ctx, 8 * (2 * (size_t)B * Wb + (size_t)B * Ws + (size_t)B));
  if (rc) return rc;
  u64* ctv = (u64*)ctx->ws.p;
  u64* sgn = ctv + (size_t)B * Wb;
  u64* small = sgn + (size_t)B * Wb;
  int64_t* v = (int64_t*)(small + (size_t)B * Ws);
  rc = fhe_linear_seeded_batch(ctx, d_body, d_id0, B, D, h_mask_key, d_w, cst - T, ctv, stream);
  if (rc) return rc;
  rc = fhe_decrypt_batch(ctx, ctv, B, v, stream);
  if (rc) return rc;
  rc = sign_extract_batch(ctx, ctv, B, sgn, small, st);
  if (rc) return rc;
  rc = fhe_decrypt_bits_batch(ctx, sgn, B, d_below, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_add_scalar, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, v, B, T, d_acc);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// ---- private-query search: an encrypted query against clear documents -----
static int query_kb(int32_t D) { return (D + 63) / 64; }
static int query_args(fhe_ctx* ctx, int64_t B, int32_t D) {
  if (B < 0 || D <= 0) return fail(ctx, FHE_E_ARG, "bad query arguments (B < 0 or D <= 0)");
  if (D > 65536) return fail(ctx, FHE_E_ARG, "query dimension D > 65536 overflows the i32 accumulators");
  return FHE_OK;
}

size_t fhe_query_docs_bytes(const fhe_params* p, int64_t B, int32_t D) {
  (void)p;  // the packing depends on the MFMA tile only, not on the scheme
  if (B < 0 || D <= 0) return 0;
  return (size_t)((B + 15) / 16) * 16 * (size_t)query_kb(D) * 64;
}

int fhe_query_docs_pack(fhe_ctx* ctx, const int64_t* d_dq, int64_t B, int32_t D, void* d_docs8, void* stream) {
  int rc = query_args(ctx, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  if (B > 0 && (!d_dq || !d_docs8)) return fail(ctx, FHE_E_ARG, "null query document buffers");
  if (B == 0) return FHE_OK;
  const int KB = query_kb(D);
  const int64_t ncb = (B + 15) / 16, lanes = ncb * KB * 64;
  if ((lanes + 255) / 256 > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "query document batch too large: split the call");
  hipLaunchKernelGGL(k_query_docs_pack, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_dq,
                     B, (int)D, KB, ncb, (v4i*)d_docs8);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_linear_query_batch(fhe_ctx* ctx, const uint64_t* d_ct_q, const void* d_docs8, int64_t B, int32_t D,
                           const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream) {
  int rc = query_args(ctx, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  if (B > 0 && (!d_ct_q || !d_docs8 || !d_w || !d_out)) return fail(ctx, FHE_E_ARG, "null linear query buffers");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const int W = p.k * p.N + 1, NB = (W + 15) / 16, KB = query_kb(D);
  const int64_t rblocks = ((B + 15) / 16 + 4 * LQ_RB - 1) / (4 * LQ_RB);
  if (rblocks > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "query document batch too large: split the call");
  // the query's byte planes: KB * 64 rows x NB * 16 columns x 8 planes
  const size_t need = (size_t)KB * 64 * NB * 16 * 8;
  if ((rc = reserve(ctx, ctx->lq_ws, need, FHE_E_DEVICE, "hipMalloc of the query plane workspace failed"))) return rc;
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_lq, st, &e1);
  ctx->prof_lq.kernel = "k_linear_query_mfma";
  hipLaunchKernelGGL(k_query_planes, dim3((unsigned)(KB * NB)), dim3(64), 0, st, d_ct_q, (int)D, W, NB, KB, d_w,
                     (v4i*)ctx->lq_ws.p);
  hipLaunchKernelGGL(k_linear_query_mfma, dim3((unsigned)rblocks, (unsigned)((NB + LQ_CB - 1) / LQ_CB)), dim3(256), 0,
                     st, (const v4i*)d_docs8, (const v4i*)ctx->lq_ws.p, B, W, NB, KB, (u64)cst << (64 - p.msg_bits),
                     d_out);
  prof_end(ctx, ctx->prof_lq, st, e1, B);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// ---- several queries of one key holder in one pass -------
static int queries_args(fhe_ctx* ctx, int64_t Q, int64_t B, int32_t D) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (Q < 1 || B < 1 || D <= 0) return fail(ctx, FHE_E_ARG, "bad queries arguments (Q < 1, B < 1 or D <= 0)");
  if (D > 65536) return fail(ctx, FHE_E_ARG, "queries dimension D > 65536 overflows the i32 accumulators");
  // the query is a grid dimension of the plane and GEMM launches
  if (Q > 65535) return fail(ctx, FHE_E_ARG, "queries batch Q > 65535: split the call");
  if (B > (int64_t)1 << 40) return fail(ctx, FHE_E_ARG, "queries document batch too large: split the call");
  return FHE_OK;
}
// n host words -> device, 32 per launch as kernel arguments (stream-ordered,
// no host buffer to keep alive, no synchronisation)
static int store_words(fhe_ctx* ctx, u64* d_dst, const u64* h_src, int64_t n, hipStream_t st) {
  for (int64_t i = 0; i < n; i += 32) {
    Words32 w;
    const int m = (int)std::min<int64_t>(32, n - i);
    for (int j = 0; j < 32; ++j) w.v[j] = j < m ? h_src[i + j] : 0;
    hipLaunchKernelGGL(k_store_words, dim3(1), dim3(64), 0, st, d_dst + i, m, w);
  }
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_linear_queries_batch(fhe_ctx* ctx, const uint64_t* d_ct_q, int64_t Q, const void* d_docs8, int64_t B,
                             int32_t D, const int64_t* d_w, const int64_t* h_cst, uint64_t* d_out, void* stream) {
  int rc = queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  if (!d_ct_q || !d_docs8 || !d_w || !h_cst || !d_out) return fail(ctx, FHE_E_ARG, "null linear queries buffers");
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const int W = p.k * p.N + 1, NB = (W + 15) / 16, KB = query_kb(D);
  const int64_t rblocks = ((B + 15) / 16 + 4 * LQ_RB - 1) / (4 * LQ_RB);
  if (rblocks > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "queries document batch too large: split the call");
  // Q plane sets (KB * 64 rows x NB * 16 columns x 8 planes each), then the Q
  // pre-scaled constants
  const size_t planes = (size_t)KB * 64 * NB * 16 * 8 * (size_t)Q, need = planes + 8 * (size_t)Q;
  if ((rc = reserve(ctx, ctx->lq_ws, need, FHE_E_NOMEM,
                    "queries plane workspace: out of device memory (fewer queries per call)")))
    return rc;
  u64* d_cst = (u64*)((char*)ctx->lq_ws.p + planes);
  std::vector<u64> cs((size_t)Q);
  for (int64_t q = 0; q < Q; ++q) cs[(size_t)q] = (u64)h_cst[q] << (64 - p.msg_bits);
  if ((rc = store_words(ctx, d_cst, cs.data(), Q, st))) return rc;
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_lq, st, &e1);
  ctx->prof_lq.kernel = "k_linear_queries_mfma";
  hipLaunchKernelGGL(k_query_planes, dim3((unsigned)(KB * NB), (unsigned)Q), dim3(64), 0, st, d_ct_q, (int)D, W, NB, KB,
                     d_w, (v4i*)ctx->lq_ws.p);
#ifdef FHEICP_LQ_QLOOP
  const unsigned qgrid = 1;  // A/B: the waves loop over the queries
#else
  const unsigned qgrid = (unsigned)Q;
#endif
  hipLaunchKernelGGL(k_linear_queries_mfma, dim3((unsigned)rblocks, (unsigned)((NB + LQ_CB - 1) / LQ_CB), qgrid),
                     dim3(256), 0, st, (const v4i*)d_docs8, (const v4i*)ctx->lq_ws.p, B, W, NB, KB, (const u64*)d_cst,
                     d_out, (int)Q);
  prof_end(ctx, ctx->prof_lq, st, e1, Q * B);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// ---- LWE -> GLWE packing key switch (k_pack.h) ------------
// gadget (beta, L) of a packing key: int8 digits, at most 8 levels, and every
// tie coin (input bit 62 - beta L - s, s < L) an input bit
static bool pack_gadget_ok(int32_t beta, int32_t L) {
  return beta >= 1 && beta <= 7 && L >= 1 && L <= 8 && beta * L + L <= 62;
}
// What tells the two gadget keys apart: where the context holds the key, its
// columns n1 ((k+1)N for the packing key, kN + 1 for the bridge key; the byte
// planes pad them to NB whole 16-column blocks) and the words of its messages.
// Each key's keygen kernel stays at its ABI entry: their arguments differ.
// For the seeded form (§8.16): the tag of the mask streams and the body of a
// row (the last `body(p)` of its n1 words: N of a GLWE row, 1 of an LWE row).
struct GadgetDesc {
  GadgetKey* (*at)(fhe_ctx*);  // the context's key, or the first of its slots
  int (*n1)(const fhe_params&);
  const char *noun, *abi;
  uint32_t tag_mask;
  int (*body)(const fhe_params&);
  int slot = 0;
  bool named = false;  // an entry that names its slot (§8.17): the slot goes into its messages
  GadgetKey& key(fhe_ctx* ctx) const { return at(ctx)[slot]; }
  int NB(const fhe_params& p) const { return (n1(p) + KSM_NB_COLS - 1) / KSM_NB_COLS; }
  size_t words(const fhe_params& p, int L) const { return (size_t)p.k * p.N * L * n1(p); }
  size_t body_words(const fhe_params& p, int L) const { return (size_t)p.k * p.N * L * body(p); }
};
static const GadgetDesc PACK_KEY = {[](fhe_ctx* c) { return &c->pack_key; }, [](const fhe_params& p) { return (p.k + 1) * p.N; }, "packing",
                                    "pack", TAG_PACK_MASK, [](const fhe_params& p) { return p.N; }};
static const GadgetDesc BRIDGE_KEY = {[](fhe_ctx* c) { return c->bridge_keys; }, [](const fhe_params& p) { return p.k * p.N + 1; }, "bridge",
                                      "bridge", TAG_BRIDGE_MASK, [](const fhe_params&) { return 1; }};

static int gadget_args(fhe_ctx* ctx, const GadgetDesc& d, int32_t beta, int32_t L) {
  if (!pack_gadget_ok(beta, L))
    return fail(ctx, FHE_E_ARG, std::string(d.noun) + " gadget out of range (1 <= base_log <= 7, 1 <= level <= 8, "
                                                      "level * (base_log + 1) <= 62)");
  return FHE_OK;
}
size_t fhe_pack_key_words(const fhe_params* p, int32_t base_log, int32_t level) {
  if (!p || !pack_gadget_ok(base_log, level)) return 0;
  return (size_t)p->k * p->N * level * (p->k + 1) * p->N;
}

// Variance the packing adds to each packed phase, in units of the integer
// words (torus variance times 2^128): the key rows' noise through the digits
// of min(count, N) inputs, plus the rounding of the input's kN mask words to
// beta L bits (half of them meet a set key bit). fheicp/params.py pack_var is
// the same expression.
static double pack_var(const fhe_params& p, int64_t count, int beta, int L) {
  const double B = std::ldexp(1.0, beta);
  const double big = (double)p.k * p.N;
  const double m = (double)std::min<int64_t>(count, p.N);
  return m * big * L * ((B * B + 2) / 12.0) * tuniform_var(p.glwe_noise_bits) +
         (1.0 + big / 2.0) * std::ldexp(1.0, 2 * (64 - beta * L)) / 12.0;
}
static double pack_sigmas(const fhe_params& p, int64_t count, double in_var, int beta, int L, int margin_log) {
  return std::ldexp(1.0, margin_log) / std::sqrt(in_var * std::ldexp(1.0, 128) + pack_var(p, count, beta, L));
}
int fhe_pack_plan(const fhe_params* params, int64_t count, double in_var, int32_t* base_log, int32_t* level,
                  int32_t* bit_levels) {
  std::string why;
  if (validate(params, why)) return fail(nullptr, FHE_E_ARG, why);
  if (count < 1 || !(in_var >= 0)) return fail(nullptr, FHE_E_ARG, "bad pack-plan arguments (count >= 1, in_var >= 0)");
  const fhe_params& p = *params;
  const int mlog = 63 - p.msg_bits;
  int bb = 0, bl = 0;
  for (int L = 1; L <= 8 && !bb; ++L)
    for (int beta = 7; beta >= 1; --beta)
      if (pack_gadget_ok(beta, L) && pack_sigmas(p, count, in_var, beta, L, mlog) >= 9.2) {
        bb = beta;
        bl = L;
        break;
      }
  if (!bb) {  // no gadget reaches the bar: the most precise one
    double best = -1;
    for (int L = 1; L <= 8; ++L)
      for (int beta = 7; beta >= 1; --beta) {
        if (!pack_gadget_ok(beta, L)) continue;
        const double sg = pack_sigmas(p, count, in_var, beta, L, mlog);
        if (sg > best) { best = sg; bb = beta; bl = L; }
      }
  }
  int lb = bl;
  for (int L = 1; L <= bl; ++L)
    if (pack_sigmas(p, count, in_var, bb, L, 62) >= 9.2) { lb = L; break; }
  if (base_log) *base_log = bb;
  if (level) *level = bl;
  if (bit_levels) *bit_levels = lb;
  return FHE_OK;
}

// (re)allocate a gadget key's buffers for L levels: 8 * words key bytes and
// kN * L rows x NB * 16 columns x 8 planes (for the packing key 8 * words too)
static int gadget_key_alloc(fhe_ctx* ctx, const GadgetDesc& d, int32_t L) {
  GadgetKey& k = d.key(ctx);
  const size_t words = d.words(ctx->p, L);
  if (k.key && d.words(ctx->p, k.level) != words) {
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipFree(k.key));
    k.key = nullptr;
    HIPCHK(ctx, hipFree(k.planes));
    k.planes = nullptr;
  }
  k.beta = k.level = 0;
  k.seeded = k.keyed = false;
  if (!k.key) {
    HIPCHK(ctx, hipMalloc(&k.key, 8 * words));
    if (hipMalloc(&k.planes, (size_t)ctx->p.k * ctx->p.N * L * d.NB(ctx->p) * KSM_NB_COLS * 8) != hipSuccess) {
      (void)hipFree(k.key);
      k.key = nullptr;
      return fail(ctx, FHE_E_DEVICE, "hipMalloc of the " + std::string(d.noun) + " key's byte planes failed");
    }
  }
  return FHE_OK;
}
// the key's 8 byte planes in B-fragment order: k_ksk_to_i8 on the layout
// [i][l][n1] with no rounding (the padded columns of a last block are zero)
static int gadget_key_planes(fhe_ctx* ctx, const GadgetDesc& d, int32_t beta, int32_t L, hipStream_t st) {
  const fhe_params& p = ctx->p;
  GadgetKey& k = d.key(ctx);
  const int big = p.k * p.N, K = big * L, n1 = d.n1(p), NB = d.NB(p);
  const int64_t tot = (int64_t)K * NB * KSM_NB_COLS;
  hipLaunchKernelGGL(k_ksk_to_i8, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, k.key, K, big, (int)L, n1, NB,
                     0, 8, k.planes);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  k.beta = beta;
  k.level = L;
  return FHE_OK;
}
static int need_gadget_key(fhe_ctx* ctx, const GadgetDesc& d) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!d.key(ctx).level && d.named)
    return fail(ctx, FHE_E_STATE, "no " + std::string(d.noun) + " key in slot " + std::to_string(d.slot) + ": call fhe_keygen_" +
                                      d.abi + "_key_slot or fhe_import_" + d.abi + "_key_slot");
  if (!d.key(ctx).level)
    return fail(ctx, FHE_E_STATE, "no " + std::string(d.noun) + " key: call fhe_keygen_" + d.abi + "_key or fhe_import_" +
                                      d.abi + "_key");
  return FHE_OK;
}
// the ABI entries' tails, after their own checks (whose order differs)
static int gadget_key_export(fhe_ctx* ctx, const GadgetDesc& d, uint64_t* h_out) {
  const GadgetKey& k = d.key(ctx);
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpy(h_out, k.key, 8 * d.words(ctx->p, k.level), hipMemcpyDeviceToHost));
  return FHE_OK;
}
static int gadget_key_import(fhe_ctx* ctx, const GadgetDesc& d, int32_t beta, int32_t L, const uint64_t* h_in) {
  int rc = gadget_key_alloc(ctx, d, L);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpy(d.key(ctx).key, h_in, 8 * d.words(ctx->p, L), hipMemcpyHostToDevice));
  return gadget_key_planes(ctx, d, beta, L, nullptr);
}

// the packing key under the context's secret: masks from Km, noise from Kn
static int keygen_pack_impl(fhe_ctx* ctx, int32_t base_log, int32_t level, const ChaKey& Km, const ChaKey& Kn,
                            hipStream_t st) {
  int rc = gadget_key_alloc(ctx, PACK_KEY, level);
  if (rc) return rc;
  const fhe_params& p = ctx->p;
  hipLaunchKernelGGL(k_keygen_pack, dim3((unsigned)(p.k * p.N * level)), dim3(256), 8 * (size_t)p.N + p.N, st, Km, Kn,
                     p.N, p.k, (int)level, (int)base_log, p.glwe_noise_bits, ctx->s_big, ctx->pack_key.key);
  HIPCHK(ctx, hipGetLastError());
  return gadget_key_planes(ctx, PACK_KEY, base_log, level, st);
}
int fhe_keygen_pack_key_key(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_key[8], void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = gadget_args(ctx, PACK_KEY, base_log, level);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_secret(ctx))) return rc;
  ChaKey K;
  if (!key_arg(h_key, K)) return fail(ctx, FHE_E_ARG, "null key");
  return keygen_pack_impl(ctx, base_log, level, K, K, (hipStream_t)stream);
}
int fhe_keygen_pack_key(fhe_ctx* ctx, int32_t base_log, int32_t level, uint64_t seed, void* stream) {
  const ChaKey K = key_from_seed(seed);
  return fhe_keygen_pack_key_key(ctx, base_log, level, K.w, stream);
}

static int need_pack_key(fhe_ctx* ctx) { return need_gadget_key(ctx, PACK_KEY); }

int fhe_export_pack_key(fhe_ctx* ctx, uint64_t* h_out) {
  int rc = need_pack_key(ctx);
  if (rc) return rc;
  if (!h_out) return fail(ctx, FHE_E_ARG, "null buffer");
  return gadget_key_export(ctx, PACK_KEY, h_out);
}

int fhe_import_pack_key(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint64_t* h_in) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = gadget_args(ctx, PACK_KEY, base_log, level);  // argument errors first
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  if (!h_in) return fail(ctx, FHE_E_ARG, "null buffer");
  return gadget_key_import(ctx, PACK_KEY, base_log, level, h_in);
}

// digits -> GEMM on the i8 matrix cores -> rotation, on the first `levels`
// levels of the key. The GEMM is the key switch's kernel on 8 planes with
// (k+1)N columns (a multiple of 16: no padded column block), K = kN * levels
// level-major, so a level prefix is a prefix of the key's k-blocks.
static int pack_impl(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int32_t levels, uint64_t* d_glwe,
                     hipStream_t st) {
  const fhe_params& p = ctx->p;
  const int big = p.k * p.N, K = big * levels, KB = K / 64, n1 = (p.k + 1) * p.N, NB = n1 / 16;
  const int64_t ncb = (count + 15) / 16, G = (count + p.N - 1) / p.N;
  if (ncb > 65535 || G * (p.N / PK_JC) > 65535) return fail(ctx, FHE_E_ARG, "pack batch too large: split the call");
  const size_t dbytes = (size_t)ncb * 16 * K, bbytes = 8 * (size_t)ncb * 16;
  const size_t need = dbytes + bbytes + 8 * (size_t)count * n1;
  int rc = reserve(ctx, ctx->pack_ws, need, FHE_E_DEVICE, "hipMalloc of the pack workspace failed");
  if (rc) return rc;
  uint32_t* Dg = (uint32_t*)ctx->pack_ws.p;
  u64* body = (u64*)((char*)ctx->pack_ws.p + dbytes);
  u64* M = (u64*)((char*)ctx->pack_ws.p + dbytes + bbytes);
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_pack, st, &e1);
  HIPCHK(ctx, hipMemsetAsync(d_glwe, 0, 8 * (size_t)G * n1, st));
  // the digits kernel also zeroes the rows the split's atomics add into
  hipLaunchKernelGGL(k_pack_digits, dim3((unsigned)(big / 64), (unsigned)ncb), dim3(256), 0, st, d_ct, count, big,
                     ctx->pack_key.beta, (int)levels, KB, Dg, body, gemm81_split(count, NB, KB).S > 1 ? n1 : 0, M);
  if ((rc = gemm81(ctx, ctx->prof_pack, "pack", Dg, ctx->pack_key.planes, body, count, n1, NB, KB, M, st))) return rc;
  hipLaunchKernelGGL(k_pack_rotate, dim3((unsigned)(p.N / 256), (unsigned)(p.k + 1), (unsigned)(G * (p.N / PK_JC))),
                     dim3(256), 0, st, M, d_ct, count, p.N, p.k, d_glwe);
  prof_end(ctx, ctx->prof_pack, st, e1, count);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_pack_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int32_t levels, uint64_t* d_glwe, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  // argument errors first: a host-only context reports them too
  if (count < 0 || levels < 0 || levels > 8) return fail(ctx, FHE_E_ARG, "bad pack arguments (count < 0 or levels outside [0, 8])");
  int rc = need_pack_key(ctx);
  if (rc) return rc;
  if (levels > ctx->pack_key.level) return fail(ctx, FHE_E_ARG, "pack levels exceed the packing key's");
  if (count > 0 && (!d_ct || !d_glwe)) return fail(ctx, FHE_E_ARG, "null pack buffers");
  if (count == 0) return FHE_OK;
  return pack_impl(ctx, d_ct, count, levels ? levels : ctx->pack_key.level, d_glwe, (hipStream_t)stream);
}

int fhe_decrypt_packed_batch(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t count, int32_t mode, int64_t* d_out,
                             void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (count < 0 || mode < 0 || mode > 2) return fail(ctx, FHE_E_ARG, "bad packed-decrypt arguments (count < 0 or mode outside 0..2)");
  int rc = need_secret(ctx);
  if (rc) return rc;
  if (count > 0 && (!d_glwe || !d_out)) return fail(ctx, FHE_E_ARG, "null packed-decrypt buffers");
  if (count == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  const int64_t G = (count + p.N - 1) / p.N;
  if (G > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "packed-decrypt batch too large: split the call");
  hipLaunchKernelGGL(k_decrypt_packed, dim3((unsigned)G), dim3(256), 8 * (size_t)p.N + p.N, (hipStream_t)stream, p.N,
                     p.k, p.msg_bits, (int)mode, ctx->s_big, d_glwe, count, d_out);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// ---- LWE -> LWE bridge key switch of a key rotation (k_bridge.h) --
// The gadget bounds are the packing key's (int8 digits, tie coins); the noise
// model is pack_var at count = 1 and the plan pack_plan's at count = 1.
size_t fhe_bridge_key_words(const fhe_params* p, int32_t base_log, int32_t level) {
  if (!p || !pack_gadget_ok(base_log, level)) return 0;
  return (size_t)p->k * p->N * level * ((size_t)p->k * p->N + 1);
}
int fhe_bridge_plan(const fhe_params* params, double in_var, int32_t* base_log, int32_t* level) {
  return fhe_pack_plan(params, 1, in_var, base_log, level, nullptr);
}

// bridge slot `slot` of a context (§8.17): BRIDGE_KEY's record on that slot
static GadgetDesc bridge_slot(int slot) {
  GadgetDesc d = BRIDGE_KEY;
  d.slot = slot;
  d.named = true;
  return d;
}
static int slot_arg(fhe_ctx* ctx, int32_t slot) {
  if (slot < 0 || slot >= FHE_BRIDGE_SLOTS)
    return fail(ctx, FHE_E_ARG, "bridge slot " + std::to_string(slot) + " outside [0, " +
                                    std::to_string(FHE_BRIDGE_SLOTS) + ")");
  return FHE_OK;
}
// the bridge key of `slot` from the old big key (kN words of 0/1, checked by
// the caller) to the context's secret: masks from Km, noise from Kn
static int keygen_bridge_impl(fhe_ctx* ctx, int slot, const uint64_t* h_s_big_old, int32_t base_log, int32_t level,
                              const ChaKey& Km, const ChaKey& Kn, hipStream_t st) {
  const fhe_params& p = ctx->p;
  const int big = p.k * p.N;
  const GadgetDesc desc = bridge_slot(slot);
  int rc = gadget_key_alloc(ctx, desc, level);
  if (rc) return rc;
  // the old secret lives on the device for this launch only
  u64* d_old = nullptr;
  HIPCHK(ctx, hipMalloc(&d_old, 8 * (size_t)big));
  hipError_t e = hipMemcpyAsync(d_old, h_s_big_old, 8 * (size_t)big, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_keygen_bridge, dim3((unsigned)(big * level)), dim3(256), 0, st, Km, Kn, big, (int)level,
                       (int)base_log, p.glwe_noise_bits, ctx->s_big, d_old, ctx->bridge_keys[slot].key);
    e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(st);
  const hipError_t e3 = hipMemset(d_old, 0, 8 * (size_t)big);
  const hipError_t e4 = hipFree(d_old);
  HIPCHK(ctx, e);
  HIPCHK(ctx, e2);
  HIPCHK(ctx, e3);
  HIPCHK(ctx, e4);
  return gadget_key_planes(ctx, desc, base_log, level, st);
}
// the argument checks of a bridge keygen, `what` in front of their messages
static int bridge_keygen_args(fhe_ctx* ctx, const uint64_t* h_s_big_old, bool keys_ok, const char* what) {
  if (!h_s_big_old || !keys_ok) return fail(ctx, FHE_E_ARG, std::string(what) + "null bridge keygen arguments");
  const int big = ctx->p.k * ctx->p.N;
  for (int i = 0; i < big; ++i)
    if (h_s_big_old[i] > 1) return fail(ctx, FHE_E_ARG, std::string(what) + "old big key word other than 0 or 1");
  return FHE_OK;
}
// the unseeded keygen of a slot; `courtesy`: refuse a key another live slot
// was generated with (the slot entries; the §8.12 entry keeps its behaviour)
static int keygen_bridge_key_at(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                                int32_t level, const uint32_t h_key[8], bool courtesy, void* stream) {
  int rc = gadget_args(ctx, BRIDGE_KEY, base_log, level);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  ChaKey K;
  if ((rc = bridge_keygen_args(ctx, h_s_big_old, key_arg(h_key, K), ""))) return rc;
  if (courtesy)
    for (int s = 0; s < FHE_BRIDGE_SLOTS; ++s) {
      const GadgetKey& o = ctx->bridge_keys[s];
      if (s != slot && o.level && o.keyed && !memcmp(o.gen.w, K.w, 32))
        return fail(ctx, FHE_E_ARG, "bridge keygen: key reuse: bridge slot " + std::to_string(s) +
                                        " of this context was generated with this key (one key serves one bridge key)");
    }
  if ((rc = need_secret(ctx))) return rc;
  if ((rc = keygen_bridge_impl(ctx, slot, h_s_big_old, base_log, level, K, K, (hipStream_t)stream))) return rc;
  ctx->bridge_keys[slot].keyed = true;
  ctx->bridge_keys[slot].gen = K;
  return FHE_OK;
}
int fhe_keygen_bridge_key_key(fhe_ctx* ctx, const uint64_t* h_s_big_old, int32_t base_log, int32_t level,
                              const uint32_t h_key[8], void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  return keygen_bridge_key_at(ctx, 0, h_s_big_old, base_log, level, h_key, false, stream);
}
int fhe_keygen_bridge_key(fhe_ctx* ctx, const uint64_t* h_s_big_old, int32_t base_log, int32_t level, uint64_t seed,
                          void* stream) {
  const ChaKey K = key_from_seed(seed);
  return fhe_keygen_bridge_key_key(ctx, h_s_big_old, base_log, level, K.w, stream);
}
int fhe_keygen_bridge_key_slot_key(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                                   int32_t level, const uint32_t h_key[8], void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  return keygen_bridge_key_at(ctx, slot, h_s_big_old, base_log, level, h_key, true, stream);
}
int fhe_keygen_bridge_key_slot(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                               int32_t level, uint64_t seed, void* stream) {
  const ChaKey K = key_from_seed(seed);
  return fhe_keygen_bridge_key_slot_key(ctx, slot, h_s_big_old, base_log, level, K.w, stream);
}

static int need_bridge_key(fhe_ctx* ctx) { return need_gadget_key(ctx, BRIDGE_KEY); }
// after the device check: the key of a slot the slot entries name
static int need_bridge_slot(fhe_ctx* ctx, int slot) { return need_gadget_key(ctx, bridge_slot(slot)); }

int fhe_export_bridge_key(fhe_ctx* ctx, uint64_t* h_out) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (!h_out) return fail(ctx, FHE_E_ARG, "null buffer");
  int rc = need_bridge_key(ctx);
  if (rc) return rc;
  return gadget_key_export(ctx, BRIDGE_KEY, h_out);
}
int fhe_export_bridge_key_slot(fhe_ctx* ctx, int32_t slot, uint64_t* h_out) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  if (!h_out) return fail(ctx, FHE_E_ARG, "null buffer");
  if ((rc = need_bridge_slot(ctx, slot))) return rc;
  return gadget_key_export(ctx, bridge_slot(slot), h_out);
}

int fhe_import_bridge_key(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint64_t* h_in) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = gadget_args(ctx, BRIDGE_KEY, base_log, level);  // argument errors first
  if (rc) return rc;
  if (!h_in) return fail(ctx, FHE_E_ARG, "null buffer");
  if ((rc = need_device(ctx))) return rc;
  return gadget_key_import(ctx, BRIDGE_KEY, base_log, level, h_in);
}
int fhe_import_bridge_key_slot(fhe_ctx* ctx, int32_t slot, int32_t base_log, int32_t level, const uint64_t* h_in) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  if ((rc = gadget_args(ctx, BRIDGE_KEY, base_log, level))) return rc;
  if (!h_in) return fail(ctx, FHE_E_ARG, "null buffer");
  if ((rc = need_device(ctx))) return rc;
  return gadget_key_import(ctx, bridge_slot(slot), base_log, level, h_in);
}
// frees a slot's words and planes; an empty slot is left as it is
int fhe_drop_bridge_key_slot(fhe_ctx* ctx, int32_t slot) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  GadgetKey& k = ctx->bridge_keys[slot];
  if (k.key || k.planes) {
    HIPCHK(ctx, hipDeviceSynchronize());  // queued work may still read the planes
    HIPCHK(ctx, hipFree(k.key));
    k.key = nullptr;
    HIPCHK(ctx, hipFree(k.planes));
    k.planes = nullptr;
  }
  k = GadgetKey{};
  return FHE_OK;
}

// digits -> GEMM on the i8 matrix cores -> copy back with the bridge key `k`,
// for the Q * B_old rows {q B + b : b < B_old} of d_in (Q x B big LWEs); row r
// of d_out takes the bridged row r (d_out may be d_in: every digit is formed
// before the copy). The GEMM is the key switch's kernel on 8 planes with
// kN + 1 columns, the same K split as pack_impl's (gemm81); it writes a
// compact count x (kN+1) buffer.
static int bridge_impl(fhe_ctx* ctx, const GadgetKey& k, const uint64_t* d_in, int64_t Q, int64_t B, int64_t B_old,
                       uint64_t* d_out, hipStream_t st) {
  const fhe_params& p = ctx->p;
  const int levels = k.level;
  const int big = p.k * p.N, K = big * levels, KB = K / 64, n1 = big + 1, NB = (n1 + KSM_NB_COLS - 1) / KSM_NB_COLS;
  const int64_t count = Q * B_old, ncb = (count + 15) / 16;
  if (ncb > 65535 || count > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "bridge batch too large: split the call");
  const size_t dbytes = (size_t)ncb * 16 * K, bbytes = 8 * (size_t)ncb * 16;
  const size_t need = dbytes + bbytes + 8 * (size_t)count * n1;
  int rc = reserve(ctx, ctx->bridge_ws, need, FHE_E_DEVICE, "hipMalloc of the bridge workspace failed");
  if (rc) return rc;
  uint32_t* Dg = (uint32_t*)ctx->bridge_ws.p;
  u64* body = (u64*)((char*)ctx->bridge_ws.p + dbytes);
  u64* M = (u64*)((char*)ctx->bridge_ws.p + dbytes + bbytes);
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_bridge, st, &e1);
  // the digits kernel also zeroes the compact rows the split's atomics add into
  hipLaunchKernelGGL(k_bridge_digits, dim3((unsigned)(big / 64), (unsigned)ncb), dim3(256), 0, st, d_in, count, B,
                     B_old, big, k.beta, levels, KB, Dg, body, gemm81_split(count, NB, KB).S > 1 ? n1 : 0, M);
  if ((rc = gemm81(ctx, ctx->prof_bridge, "bridge", Dg, k.planes, body, count, n1, NB, KB, M, st))) return rc;
  hipLaunchKernelGGL(k_bridge_scatter, dim3((unsigned)count, (unsigned)((n1 + 255) / 256)), dim3(256), 0, st, M, count,
                     B, B_old, n1, d_out);
  prof_end(ctx, ctx->prof_bridge, st, e1, count);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_bridge_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, uint64_t* d_out, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  // argument errors first: a host-only context reports them too
  if (count < 0) return fail(ctx, FHE_E_ARG, "bad bridge arguments (count < 0)");
  if (count > 0 && (!d_ct || !d_out)) return fail(ctx, FHE_E_ARG, "null bridge buffers");
  int rc = need_bridge_key(ctx);
  if (rc) return rc;
  if (count == 0) return FHE_OK;
  return bridge_impl(ctx, ctx->bridge_keys[0], d_ct, 1, count, count, d_out, (hipStream_t)stream);
}

int fhe_bridge_rows_batch(fhe_ctx* ctx, uint64_t* d_ct, int64_t Q, int64_t B, int64_t B_old, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  // argument errors first: a host-only context reports them too
  if (Q < 1 || B < 1 || Q > 0x7fffffffLL || B > 0x7fffffffLL || Q * B > 0x7fffffffLL)
    return fail(ctx, FHE_E_ARG, "bad bridge rows arguments (Q < 1, B < 1 or Q*B >= 2^31)");
  if (B_old < 0 || B_old > B) return fail(ctx, FHE_E_ARG, "bad bridge rows arguments (B_old outside [0, B])");
  if (!d_ct) return fail(ctx, FHE_E_ARG, "null bridge buffers");
  int rc = need_bridge_key(ctx);
  if (rc) return rc;
  if (B_old == 0) return FHE_OK;
  return bridge_impl(ctx, ctx->bridge_keys[0], d_ct, Q, B, B_old, d_ct, (hipStream_t)stream);
}

// ---- several old generations resident: the generation row map (§8.17) -----
#ifndef FHEICP_GRP_BRIDGE
#define FHEICP_GRP_BRIDGE 1  // 0: one single-key bridge per generation behind the same entries (A/B builds,
                             // tools/build_variant.sh NAME -DFHEICP_GRP_BRIDGE=0; the fallback)
#endif
// the row map's argument checks: FHE_E_ARG, on host-only contexts too
static int gens_args(fhe_ctx* ctx, int64_t B, int32_t G, const int64_t* h_ends, const int32_t* h_slots) {
  if (G < 0 || G > FHE_BRIDGE_SLOTS)
    return fail(ctx, FHE_E_ARG, "bad bridge generations arguments (G outside [0, " +
                                    std::to_string(FHE_BRIDGE_SLOTS) + "])");
  if (G > 0 && (!h_ends || !h_slots)) return fail(ctx, FHE_E_ARG, "null bridge generations tables");
  int64_t prev = 0;
  uint32_t seen = 0;
  for (int g = 0; g < G; ++g) {
    if (h_ends[g] < prev || h_ends[g] > B)
      return fail(ctx, FHE_E_ARG, "bad bridge generations arguments (ends must not decrease and stay within [0, B])");
    prev = h_ends[g];
    int rc = slot_arg(ctx, h_slots[g]);
    if (rc) return rc;
    if (seen >> h_slots[g] & 1)
      return fail(ctx, FHE_E_ARG, "bad bridge generations arguments (bridge slot " + std::to_string(h_slots[g]) +
                                      " named twice)");
    seen |= 1u << h_slots[g];
  }
  return FHE_OK;
}
extern "C++" {
// The generations with documents of a row map, oldest first: f(slot, d0, n)
// for the n documents from d0 on; stops at the first nonzero return.
template <typename F>
static int for_gens(int32_t G, const int64_t* h_ends, const int32_t* h_slots, F&& f) {
  for (int g = 0; g < G; ++g) {
    const int64_t d0 = g ? h_ends[g - 1] : 0, n = h_ends[g] - d0;
    if (n == 0) continue;
    if (int rc = f((int)h_slots[g], d0, n)) return rc;
  }
  return FHE_OK;
}
// The same walk after the device check, with the key checks of a generation
// before f(slot, key, d0, n) sees it: its slot holds a key (need_bridge_slot's
// code and message) and that key has the gadget of the first such generation's
// (FHE_E_STATE; the first is named by its slot when name_first). err(code,
// message) words the context and returns the code.
template <typename Err, typename F>
static int for_gen_keys(fhe_ctx* ctx, int32_t G, const int64_t* h_ends, const int32_t* h_slots, bool name_first,
                        Err&& err, F&& f) {
  const GadgetKey* first = nullptr;
  int first_slot = 0;
  return for_gens(G, h_ends, h_slots, [&](int slot, int64_t d0, int64_t n) {
    int rc = need_bridge_slot(ctx, slot);
    if (rc) return err(rc, std::string(fhe_last_error(ctx)));
    const GadgetKey& k = ctx->bridge_keys[slot];
    if (!first) first = &k, first_slot = slot;
    if (k.beta != first->beta || k.level != first->level)
      return err(FHE_E_STATE,
                 "bridge gadgets differ: slot " + std::to_string(slot) + " holds (" + std::to_string(k.beta) + ", " +
                     std::to_string(k.level) + "), " +
                     (name_first ? "slot " + std::to_string(first_slot) : std::string("an earlier generation's slot")) +
                     " (" + std::to_string(first->beta) + ", " + std::to_string(first->level) + ")");
    return f(slot, k, d0, n);
  });
}
}  // extern "C++"
static size_t up16(size_t x) { return (x + 15) / 16 * 16; }
// One segmented pass (k_bridge.h): the segments whose keys share the gadget
// (beta, level), a key's byte planes each, and what they add up to in blocks
// of 128 rows, digit groups of 16 rows and compact rows.
struct BridgePass {
  int beta = 0, level = 0;
  int64_t nblk = 0, ndg = 0, rows = 0;
  std::vector<BridgeSeg> segs;
  std::vector<const void*> planes;
  // the n > 0 documents from doc0 on of a Q x B result at buffer row row0
  void add(int64_t Q, int64_t n, int64_t doc0, int64_t B, int64_t row0, const void* key_planes) {
    segs.push_back(BridgeSeg{rows, n, doc0, B, row0});
    planes.push_back(key_planes);
    rows += Q * n;
    nblk += (Q * n + KSM_CTS - 1) / KSM_CTS;
    ndg += (Q * n + 15) / 16;
  }
  bool fits() const { return ndg <= 65535 && 8 * nblk <= 65535; }  // the launches' grid limits
  // the workspace: starts | ends | the segment records | the key table | the
  // block table | digits | bodies | the compact result
  void layout(int big, size_t off[5]) const {
    off[0] = up16(8 * segs.size() * (3 + BRIDGE_SEG_WORDS));        // the block table
    off[1] = off[0] + up16(sizeof(KsGrpBlock) * (size_t)nblk);      // digits
    off[2] = off[1] + (size_t)ndg * 16 * (size_t)(big * level);     // bodies
    off[3] = off[2] + up16(8 * (size_t)rows);                       // the compact result
    off[4] = off[3] + 8 * (size_t)rows * (size_t)(big + 1);
  }
};
// One pass on the rows of d_ct, in place, in the workspace w of layout()'s
// off[4] bytes: the tables (store_words in stream order, then the block
// table), the digits, the group GEMM and the copy back. One bracket in ctx's
// "bridge" bucket, items = the pass's rows.
static int bridge_pass_launch(fhe_ctx* ctx, char* w, u64* d_ct, const BridgePass& ps, hipStream_t st) {
  const int big = ctx->p.k * ctx->p.N, n1 = big + 1, NB = (n1 + KSM_NB_COLS - 1) / KSM_NB_COLS;
  const size_t S = ps.segs.size();
  size_t off[5];
  ps.layout(big, off);
  std::vector<u64> words(S * (3 + BRIDGE_SEG_WORDS));
  for (size_t s = 0; s < S; ++s) {
    const BridgeSeg& sg = ps.segs[s];
    words[s] = (u64)sg.start;
    words[S + s] = (u64)(s + 1 < S ? ps.segs[s + 1].start : ps.rows);  // segments follow each other unpadded
    memcpy(&words[2 * S + s * BRIDGE_SEG_WORDS], &sg, sizeof(BridgeSeg));
    words[(2 + BRIDGE_SEG_WORDS) * S + s] = (u64)(uintptr_t)ps.planes[s];
  }
  int64_t* se = (int64_t*)w;
  BridgeSeg* seg = (BridgeSeg*)(se + 2 * S);
  const void** keys = (const void**)(se + (2 + BRIDGE_SEG_WORDS) * S);
  KsGrpBlock* blk = (KsGrpBlock*)(w + off[0]);
  uint32_t* Dg = (uint32_t*)(w + off[1]);
  u64* body = (u64*)(w + off[2]);
  u64* M = (u64*)(w + off[3]);
  const int KB = big * ps.level / 64;
  // the single bridge's split rule on the launch's blocks x column blocks
  const auto [Sk, kslice] = ksm_split(KB, ps.nblk * NB, 512);
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_bridge, st, &e1);
  int rc = store_words(ctx, (u64*)w, words.data(), (int64_t)words.size(), st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ks_grp_tables, dim3((unsigned)((ps.nblk + 255) / 256)), dim3(256), 0, st, (const int64_t*)se,
                     (int)S, ps.nblk, blk);
  // the digits kernel also zeroes the compact rows the split's atomics add into
  hipLaunchKernelGGL(k_bridge_digits_seg, dim3((unsigned)(big / 64), (unsigned)(8 * ps.nblk)), dim3(256), 0, st,
                     (const u64*)d_ct, (const KsGrpBlock*)blk, (const BridgeSeg*)seg, big, ps.beta, ps.level, KB, Dg,
                     body, Sk > 1 ? n1 : 0, M);
  ctx->prof_bridge.kernel = "k_keyswitch_mfma_grp<8, 1>";
  hipLaunchKernelGGL((k_keyswitch_mfma_grp<8, 1>), dim3((unsigned)(ps.nblk * NB * Sk)), dim3(256), 0, st,
                     (const v4i*)Dg, (const v4i* const*)keys, (const KsGrpBlock*)blk, (const u64*)body, n1, NB, KB, 0,
                     Sk, kslice, M);
  hipLaunchKernelGGL(k_bridge_scatter_seg, dim3((unsigned)(8 * ps.nblk), (unsigned)((n1 + 255) / 256)), dim3(256), 0,
                     st, (const u64*)M, (const KsGrpBlock*)blk, (const BridgeSeg*)seg, n1, d_ct);
  prof_end(ctx, ctx->prof_bridge, st, e1, ps.rows);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
// a context's row map as one pass: a segment per generation with documents,
// row0 = 0 (the keys are in place: after gens_ready's checks)
static BridgePass gens_pass(fhe_ctx* ctx, int64_t Q, int64_t B, int32_t G, const int64_t* h_ends,
                            const int32_t* h_slots) {
  BridgePass ps;
  for_gens(G, h_ends, h_slots, [&](int slot, int64_t d0, int64_t n) {
    const GadgetKey& k = ctx->bridge_keys[slot];
    ps.beta = k.beta, ps.level = k.level;
    ps.add(Q, n, d0, B, 0, k.planes);
    return (int)FHE_OK;
  });
  return ps;
}
// After the device check and before anything is queued: every named slot with
// rows holds a key (FHE_E_STATE naming the slot), those keys share one gadget
// (FHE_E_STATE), and the launch limits hold (FHE_E_ARG; the segmented pass's
// over all generations, the loop's per generation).
static int gens_ready(fhe_ctx* ctx, int64_t Q, int64_t B, int32_t G, const int64_t* h_ends, const int32_t* h_slots) {
  int rc = for_gen_keys(
      ctx, G, h_ends, h_slots, false, [&](int code, const std::string& msg) { return fail(ctx, code, msg); },
      [&](int, const GadgetKey&, int64_t, int64_t n) {
        if (!FHEICP_GRP_BRIDGE && (Q * n + 15) / 16 > 65535)
          return fail(ctx, FHE_E_ARG, "bridge batch too large: split the call");
        return (int)FHE_OK;
      });
  if (rc) return rc;
  if (FHEICP_GRP_BRIDGE && !gens_pass(ctx, Q, B, G, h_ends, h_slots).fits())
    return fail(ctx, FHE_E_ARG, "bridge batch too large (more than 65535 digit groups of 16 rows, or 8191 blocks of "
                                "128 rows, over all generations): split the call");
  return FHE_OK;
}
// The bridge of every generation's rows of d_ct (Q x B big LWEs, in place),
// after gens_args and gens_ready: one segmented pass in ctx->bridge_ws.
static int bridge_gens_impl(fhe_ctx* ctx, uint64_t* d_ct, int64_t Q, int64_t B, int32_t G, const int64_t* h_ends,
                            const int32_t* h_slots, hipStream_t st) {
  const int big = ctx->p.k * ctx->p.N;
  if (!FHEICP_GRP_BRIDGE)
    return for_gens(G, h_ends, h_slots, [&](int slot, int64_t d0, int64_t n) {
      // the single bridge's row map on the rows from document d0 on: row q B + j there is row q B + d0 + j here
      u64* base = d_ct + (size_t)d0 * (big + 1);
      return bridge_impl(ctx, ctx->bridge_keys[slot], base, Q, B, n, base, st);
    });
  const BridgePass ps = gens_pass(ctx, Q, B, G, h_ends, h_slots);
  if (ps.rows == 0) return FHE_OK;
  size_t off[5];
  ps.layout(big, off);
  int rc = reserve(ctx, ctx->bridge_ws, off[4], FHE_E_DEVICE, "hipMalloc of the bridge workspace failed");
  if (rc) return rc;
  return bridge_pass_launch(ctx, (char*)ctx->bridge_ws.p, d_ct, ps, st);
}

int fhe_bridge_gens_batch(fhe_ctx* ctx, uint64_t* d_ct, int64_t Q, int64_t B, int32_t G, const int64_t* h_ends,
                          const int32_t* h_slots, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  // argument errors first: a host-only context reports them too
  if (Q < 1 || B < 1 || Q > 0x7fffffffLL || B > 0x7fffffffLL || Q * B > 0x7fffffffLL)
    return fail(ctx, FHE_E_ARG, "bad bridge generations arguments (Q < 1, B < 1 or Q*B >= 2^31)");
  int rc = gens_args(ctx, B, G, h_ends, h_slots);
  if (rc) return rc;
  if (!d_ct) return fail(ctx, FHE_E_ARG, "null bridge buffers");
  if ((rc = need_device(ctx))) return rc;
  if ((rc = gens_ready(ctx, Q, B, G, h_ends, h_slots))) return rc;
  return bridge_gens_impl(ctx, d_ct, Q, B, G, h_ends, h_slots, (hipStream_t)stream);
}

// The leveled part of a private-query search, shared by the single-party
// compare and the two-party server entry: the workspace
//   ct_v (B big) | sign (B big) | small (B) | v (B) | the query's D expanded
//   ciphertexts | its stream id | (keep_copy: a second B big)
// then the query's expansion and the GEMM with cst on the body, into ct_v.
struct QueryWs {
  u64 *ctv, *sgn, *small;
  int64_t* v;
  u64* cpy;
};
// the workspace above with `extra` words in the query's place
static int leveled_ws(fhe_ctx* ctx, int64_t B, size_t extra, bool keep_copy, QueryWs* w, u64** d_extra) {
  const fhe_params& p = ctx->p;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
  int rc = ensure_ws(ctx, 8 * (2 * (size_t)B * Wb + (size_t)B * Ws + (size_t)B + extra +
                               (keep_copy ? (size_t)B * Wb : 0)));
  if (rc) return rc;
  w->ctv = (u64*)ctx->ws.p;
  w->sgn = w->ctv + (size_t)B * Wb;
  w->small = w->sgn + (size_t)B * Wb;
  w->v = (int64_t*)(w->small + (size_t)B * Ws);
  u64* ex = (u64*)(w->v + B);
  if (d_extra) *d_extra = ex;
  w->cpy = keep_copy ? ex + extra : nullptr;
  return FHE_OK;
}
static int query_leveled(fhe_ctx* ctx, const uint64_t* d_qbody, uint64_t id0, const uint32_t h_mask_key[8],
                         const void* d_docs8, int64_t B, int32_t D, const int64_t* d_w, int64_t cst, bool keep_copy,
                         QueryWs* w, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t Wb = fhe_big_lwe_words(&ctx->p);
  u64* ctq;
  int rc = leveled_ws(ctx, B, (size_t)D * Wb + 1, keep_copy, w, &ctq);
  if (rc) return rc;
  u64* idw = ctq + (size_t)D * Wb;
  hipLaunchKernelGGL(k_store_word, dim3(1), dim3(64), 0, st, idw, (u64)id0);
  HIPCHK(ctx, hipGetLastError());
  rc = fhe_expand_seeded_batch(ctx, d_qbody, idw, 1, D, h_mask_key, ctq, stream);
  if (rc) return rc;
  return fhe_linear_query_batch(ctx, ctq, d_docs8, B, D, d_w, cst, w->ctv, stream);
}

// What follows the leveled step, shared by the private-query and the
// both-private entries. Single party: decrypt the leveled accumulator of
// acc - T, sign extraction, decrypt the threshold bit, add T back.
static int post_leveled_compare(fhe_ctx* ctx, const QueryWs& w, int64_t B, int64_t T, int64_t* d_acc,
                                int64_t* d_below, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = fhe_decrypt_batch(ctx, w.ctv, B, w.v, stream);
  if (rc) return rc;
  rc = sign_extract_batch(ctx, w.ctv, B, w.sgn, w.small, st);
  if (rc) return rc;
  rc = fhe_decrypt_bits_batch(ctx, w.sgn, B, d_below, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_add_scalar, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, w.v, B, T, d_acc);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
// Evaluation-only server: copy the leveled ciphertexts (the sign extraction
// consumes them), sign extraction, pack the copies with every level and the
// sign ciphertexts with the first levels_bit levels (0: all).
static int post_leveled_search(fhe_ctx* ctx, const QueryWs& w, int64_t B, int32_t levels_bit, uint64_t* d_glwe_acc,
                               uint64_t* d_glwe_bit, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t Wb = fhe_big_lwe_words(&ctx->p);
  HIPCHK(ctx, hipMemcpyAsync(w.cpy, w.ctv, 8 * (size_t)B * Wb, hipMemcpyDeviceToDevice, st));
  int rc = sign_extract_batch(ctx, w.ctv, B, w.sgn, w.small, st);
  if (rc) return rc;
  rc = pack_impl(ctx, w.cpy, B, ctx->pack_key.level, d_glwe_acc, st);
  if (rc) return rc;
  return pack_impl(ctx, w.sgn, B, levels_bit ? levels_bit : ctx->pack_key.level, d_glwe_bit, st);
}

int fhe_compare_query_batch(fhe_ctx* ctx, const uint64_t* d_qbody, uint64_t id0, const uint32_t h_mask_key[8],
                            const void* d_docs8, int64_t B, int32_t D, const int64_t* d_w, int64_t cst, int64_t T,
                            int64_t* d_acc, int64_t* d_below, void* stream) {
  int rc = query_args(ctx, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_secret(ctx))) return rc;
  if (!h_mask_key || (B > 0 && (!d_qbody || !d_docs8 || !d_w || !d_acc || !d_below)))
    return fail(ctx, FHE_E_ARG, "null compare query arguments");
  if (B == 0) return FHE_OK;
  QueryWs w;
  rc = query_leveled(ctx, d_qbody, id0, h_mask_key, d_docs8, B, D, d_w, cst - T, false, &w, stream);
  if (rc) return rc;
  return post_leveled_compare(ctx, w, B, T, d_acc, d_below, stream);
}

// The server of the two-party private query: the pipeline of
// fhe_compare_query_batch without either decryption. The leveled ciphertexts
// of acc - T are copied (the sign extraction consumes them) and packed with
// every level; the sign ciphertexts with the first levels_bit levels (0: all).
// Needs the evaluation keys and the packing key only.
int fhe_search_query_batch(fhe_ctx* ctx, const uint64_t* d_qbody, uint64_t id0, const uint32_t h_mask_key[8],
                           const void* d_docs8, int64_t B, int32_t D, const int64_t* d_w, int64_t cst, int64_t T,
                           int32_t levels_bit, uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream) {
  int rc = query_args(ctx, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8) return fail(ctx, FHE_E_ARG, "bad search query arguments (levels_bit outside [0, 8])");
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if (levels_bit > ctx->pack_key.level) return fail(ctx, FHE_E_ARG, "search query levels_bit exceeds the packing key's levels");
  if (!h_mask_key || (B > 0 && (!d_qbody || !d_docs8 || !d_w || !d_glwe_acc || !d_glwe_bit)))
    return fail(ctx, FHE_E_ARG, "null search query arguments");
  if (B == 0) return FHE_OK;
  QueryWs w;
  rc = query_leveled(ctx, d_qbody, id0, h_mask_key, d_docs8, B, D, d_w, cst - T, true, &w, stream);
  if (rc) return rc;
  return post_leveled_search(ctx, w, B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}

// post_leveled_compare over the Q B query-major ciphertexts of a batch, with
// query q's own threshold (d_T[q], device) added back: shared by the
// private-query (§8.8) and the stored-ciphertext (§8.9) batched entries.
static int post_leveled_compare_queries(fhe_ctx* ctx, const QueryWs& w, int64_t Q, int64_t B, const int64_t* d_T,
                                        int64_t* d_acc, int64_t* d_below, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = Q * B;
  int rc;
  if ((rc = fhe_decrypt_batch(ctx, w.ctv, n, w.v, stream))) return rc;
  if ((rc = sign_extract_batch(ctx, w.ctv, n, w.sgn, w.small, st))) return rc;
  if ((rc = fhe_decrypt_bits_batch(ctx, w.sgn, n, d_below, stream))) return rc;
  hipLaunchKernelGGL(k_add_query_scalar, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w.v, n, B, d_T, d_acc);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// Q queries of one key holder in one pass: the workspace of
// query_leveled for Q B results with, in the query's place, the Q D expanded
// ciphertexts and the Q thresholds; one expansion (k_expand_seeded's B = Q),
// one GEMM launch with cst - T_q on query q's bodies, into ct_v (query-major).
static int queries_leveled(fhe_ctx* ctx, const uint64_t* d_qbody, const uint64_t* d_id0, const uint32_t h_mask_key[8],
                           int64_t Q, const void* d_docs8, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                           const int64_t* h_T, bool keep_copy, QueryWs* w, int64_t** d_T, void* stream) {
  const size_t Wb = fhe_big_lwe_words(&ctx->p);
  u64* ctq;
  int rc = leveled_ws(ctx, Q * B, (size_t)Q * D * Wb + (size_t)Q, keep_copy, w, &ctq);
  if (rc) return rc;
  *d_T = (int64_t*)(ctq + (size_t)Q * D * Wb);
  std::vector<int64_t> cs((size_t)Q);
  for (int64_t q = 0; q < Q; ++q) cs[(size_t)q] = cst - h_T[q];
  if ((rc = store_words(ctx, (u64*)*d_T, (const u64*)h_T, Q, (hipStream_t)stream))) return rc;
  rc = fhe_expand_seeded_batch(ctx, d_qbody, d_id0, Q, D, h_mask_key, ctq, stream);
  if (rc) return rc;
  return fhe_linear_queries_batch(ctx, ctq, Q, d_docs8, B, D, d_w, cs.data(), w->ctv, stream);
}

int fhe_compare_queries_batch(fhe_ctx* ctx, const uint64_t* d_qbody, const uint64_t* d_id0,
                              const uint32_t h_mask_key[8], int64_t Q, const void* d_docs8, int64_t B, int32_t D,
                              const int64_t* d_w, int64_t cst, const int64_t* h_T, int64_t* d_acc, int64_t* d_below,
                              void* stream) {
  int rc = queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_secret(ctx))) return rc;
  if (!h_mask_key || !h_T || !d_qbody || !d_id0 || !d_docs8 || !d_w || !d_acc || !d_below)
    return fail(ctx, FHE_E_ARG, "null compare queries arguments");
  QueryWs w;
  int64_t* d_T;
  rc = queries_leveled(ctx, d_qbody, d_id0, h_mask_key, Q, d_docs8, B, D, d_w, cst, h_T, false, &w, &d_T, stream);
  if (rc) return rc;
  return post_leveled_compare_queries(ctx, w, Q, B, d_T, d_acc, d_below, stream);
}

int fhe_search_queries_batch(fhe_ctx* ctx, const uint64_t* d_qbody, const uint64_t* d_id0,
                             const uint32_t h_mask_key[8], int64_t Q, const void* d_docs8, int64_t B, int32_t D,
                             const int64_t* d_w, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                             uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream) {
  int rc = queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad search queries arguments (levels_bit outside [0, 8])");
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if (levels_bit > ctx->pack_key.level)
    return fail(ctx, FHE_E_ARG, "search queries levels_bit exceeds the packing key's levels");
  if (!h_mask_key || !h_T || !d_qbody || !d_id0 || !d_docs8 || !d_w || !d_glwe_acc || !d_glwe_bit)
    return fail(ctx, FHE_E_ARG, "null search queries arguments");
  QueryWs w;
  int64_t* d_T;
  rc = queries_leveled(ctx, d_qbody, d_id0, h_mask_key, Q, d_docs8, B, D, d_w, cst, h_T, true, &w, &d_T, stream);
  if (rc) return rc;
  // result q B + b is ciphertext q B + b of the batch: coefficient (q B + b) mod N
  // of GLWE (q B + b) / N
  return post_leveled_search(ctx, w, Q * B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}

// ---- stored-ciphertext search: Q clear queries in one pass --
static int seeded_queries_args(fhe_ctx* ctx, int64_t Q, int64_t B, int32_t D) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (Q < 1 || B < 1 || D < 1) return fail(ctx, FHE_E_ARG, "bad seeded queries arguments (Q < 1, B < 1 or D < 1)");
  // the query tile is a grid dimension of the leveled launch
  if (Q > 65535) return fail(ctx, FHE_E_ARG, "seeded queries batch Q > 65535: split the call");
  if (B > 0x7fffffffLL || B * (int64_t)D > 0x7fffffffLL)
    return fail(ctx, FHE_E_ARG, "seeded queries corpus batch too large (B*D >= 2^31)");
  if (Q * B > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "seeded queries result count too large (Q*B >= 2^31)");
  return FHE_OK;
}
// the leveled launch: d_cst holds the Q scaled constants on the device
static int linear_seeded_queries_launch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                        int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                        const u64* d_cst, uint64_t* d_out, hipStream_t st) {
  const fhe_params& p = ctx->p;
  ChaKey Km;
  for (int i = 0; i < 8; ++i) Km.w[i] = h_mask_key[i];
  constexpr int QT = FHEICP_LSQ_QT;
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_ls, st, &e1);
  ctx->prof_ls.kernel = "k_linear_seeded_queries";
  hipLaunchKernelGGL(k_linear_seeded_queries<QT>, dim3((unsigned)B, (unsigned)((Q + QT - 1) / QT)), dim3(256), 0, st,
                     Km, p.k * p.N, d_body, d_id0, (int)D, (int)Q, d_W, d_cst, d_out);
  prof_end(ctx, ctx->prof_ls, st, e1, Q * B);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
// h_cst[q] (minus h_T[q] when given) scaled to the encoding, to d_cst through k_store_words
static int store_scaled_csts(fhe_ctx* ctx, u64* d_cst, int64_t Q, const int64_t* h_cst, int64_t cst,
                             const int64_t* h_T, hipStream_t st) {
  std::vector<u64> cs((size_t)Q);
  for (int64_t q = 0; q < Q; ++q)
    cs[(size_t)q] = (u64)(h_cst ? h_cst[q] : cst - h_T[q]) << (64 - ctx->p.msg_bits);
  return store_words(ctx, d_cst, cs.data(), Q, st);
}

int fhe_linear_seeded_queries_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                                    const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                    const int64_t* h_cst, uint64_t* d_out, void* stream) {
  int rc = seeded_queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (!d_body || !d_id0 || !h_mask_key || !d_W || !h_cst || !d_out)
    return fail(ctx, FHE_E_ARG, "null linear seeded queries arguments");
  if ((rc = need_device(ctx))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = reserve(ctx, ctx->lsq_cst, 8 * (size_t)Q, FHE_E_DEVICE, "hipMalloc of the scaled constants failed")))
    return rc;
  if ((rc = store_scaled_csts(ctx, (u64*)ctx->lsq_cst.p, Q, h_cst, 0, nullptr, st))) return rc;
  return linear_seeded_queries_launch(ctx, d_body, d_id0, B, D, h_mask_key, Q, d_W, (const u64*)ctx->lsq_cst.p, d_out,
                                      st);
}

// The leveled part of the compare and search entries: the workspace of the
// §8.8 entries for Q B results with, in the query's place, the Q thresholds
// and the Q scaled constants cst - T_q; one launch into ct_v (query-major).
static int seeded_queries_leveled(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                                  const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W, int64_t cst,
                                  const int64_t* h_T, bool keep_copy, QueryWs* w, int64_t** d_T, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  u64* ex;
  int rc = leveled_ws(ctx, Q * B, 2 * (size_t)Q, keep_copy, w, &ex);
  if (rc) return rc;
  *d_T = (int64_t*)ex;
  if ((rc = store_words(ctx, ex, (const u64*)h_T, Q, st))) return rc;
  if ((rc = store_scaled_csts(ctx, ex + Q, Q, nullptr, cst, h_T, st))) return rc;
  return linear_seeded_queries_launch(ctx, d_body, d_id0, B, D, h_mask_key, Q, d_W, ex + Q, w->ctv, st);
}

int fhe_compare_seeded_queries_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                     int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                     int64_t cst, const int64_t* h_T, int64_t* d_acc, int64_t* d_below,
                                     void* stream) {
  int rc = seeded_queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (!d_body || !d_id0 || !h_mask_key || !d_W || !h_T || !d_acc || !d_below)
    return fail(ctx, FHE_E_ARG, "null compare seeded queries arguments");
  if ((rc = need_secret(ctx))) return rc;
  QueryWs w;
  int64_t* d_T;
  rc = seeded_queries_leveled(ctx, d_body, d_id0, B, D, h_mask_key, Q, d_W, cst, h_T, false, &w, &d_T, stream);
  if (rc) return rc;
  return post_leveled_compare_queries(ctx, w, Q, B, d_T, d_acc, d_below, stream);
}

// The evaluation-only entry with the first B_old documents under a rotated-out
// key: their rows {q B + b : b < B_old} of the leveled result
// are bridged in place before the copy is taken. B_old = 0: no bridge, no
// bridge key needed.
int fhe_search_seeded_queries_bridged_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                            int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                            int64_t cst, const int64_t* h_T, int32_t levels_bit, int64_t B_old,
                                            uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream) {
  int rc = seeded_queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad search seeded queries arguments (levels_bit outside [0, 8])");
  if (!d_body || !d_id0 || !h_mask_key || !d_W || !h_T || !d_glwe_acc || !d_glwe_bit)
    return fail(ctx, FHE_E_ARG, "null search seeded queries arguments");
  if (B_old < 0 || B_old > B) return fail(ctx, FHE_E_ARG, "bad search seeded queries arguments (B_old outside [0, B])");
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if (B_old > 0 && (rc = need_bridge_key(ctx))) return rc;
  if (levels_bit > ctx->pack_key.level)
    return fail(ctx, FHE_E_ARG, "search seeded queries levels_bit exceeds the packing key's levels");
  QueryWs w;
  int64_t* d_T;
  rc = seeded_queries_leveled(ctx, d_body, d_id0, B, D, h_mask_key, Q, d_W, cst, h_T, true, &w, &d_T, stream);
  if (rc) return rc;
  if (B_old > 0 && (rc = bridge_impl(ctx, ctx->bridge_keys[0], w.ctv, Q, B, B_old, w.ctv, (hipStream_t)stream)))
    return rc;
  return post_leveled_search(ctx, w, Q * B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}

// The same entry with several old generations resident:
// the generation row map (G, h_ends, h_slots) in B_old's place; documents
// b >= h_ends[G - 1] are under the current key. G = 0: no bridge, no bridge
// key needed.
int fhe_search_seeded_queries_gens_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                         int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                         int64_t cst, const int64_t* h_T, int32_t levels_bit, int32_t G,
                                         const int64_t* h_ends, const int32_t* h_slots, uint64_t* d_glwe_acc,
                                         uint64_t* d_glwe_bit, void* stream) {
  int rc = seeded_queries_args(ctx, Q, B, D);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad search seeded queries arguments (levels_bit outside [0, 8])");
  if (!d_body || !d_id0 || !h_mask_key || !d_W || !h_T || !d_glwe_acc || !d_glwe_bit)
    return fail(ctx, FHE_E_ARG, "null search seeded queries arguments");
  if ((rc = gens_args(ctx, B, G, h_ends, h_slots))) return rc;
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if ((rc = gens_ready(ctx, Q, B, G, h_ends, h_slots))) return rc;
  if (levels_bit > ctx->pack_key.level)
    return fail(ctx, FHE_E_ARG, "search seeded queries levels_bit exceeds the packing key's levels");
  QueryWs w;
  int64_t* d_T;
  rc = seeded_queries_leveled(ctx, d_body, d_id0, B, D, h_mask_key, Q, d_W, cst, h_T, true, &w, &d_T, stream);
  if (rc) return rc;
  if ((rc = bridge_gens_impl(ctx, w.ctv, Q, B, G, h_ends, h_slots, (hipStream_t)stream))) return rc;
  return post_leveled_search(ctx, w, Q * B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}

int fhe_search_seeded_queries_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                    int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                    int64_t cst, const int64_t* h_T, int32_t levels_bit, uint64_t* d_glwe_acc,
                                    uint64_t* d_glwe_bit, void* stream) {
  return fhe_search_seeded_queries_bridged_batch(ctx, d_body, d_id0, B, D, h_mask_key, Q, d_W, cst, h_T, levels_bit, 0,
                                                 d_glwe_acc, d_glwe_bit, stream);
}

// ---- both-private search: GGSW query x GLWE documents (k_extprod.h, §8.7) --
// the gadget bounds are the packing key switch's (int8 digits, tie coins)
static int ggsw_args(fhe_ctx* ctx, int64_t B, int32_t D, int32_t beta, int32_t L) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (B < 0 || D <= 0) return fail(ctx, FHE_E_ARG, "bad ggsw arguments (B < 0 or D <= 0)");
  if (D > ctx->p.N) return fail(ctx, FHE_E_ARG, "ggsw dimension D > N: a document must fit one GLWE");
  if (!pack_gadget_ok(beta, L))
    return fail(ctx, FHE_E_ARG, "ggsw gadget out of range (1 <= base_log <= 7, 1 <= level <= 8, "
                                "level * (base_log + 1) <= 62)");
  return FHE_OK;
}
size_t fhe_ggsw_words(const fhe_params* p, int32_t base_log, int32_t level) {
  if (!p || !pack_gadget_ok(base_log, level)) return 0;
  return (size_t)(p->k + 1) * level * (p->k + 1) * p->N;
}

// Variance of an extracted phase, integer-word units: the GGSW rows' noise
// through the (noiseless) message and through the digits, plus the rounding
// of the document's (k+1)N words to beta L bits times the query polynomial.
// fheicp/params.py extprod_var is the same expression.
static double extprod_var(const fhe_params& p, double w2, int beta, int L) {
  const double B = std::ldexp(1.0, beta), tv = tuniform_var(p.glwe_noise_bits);
  return w2 * tv + (double)(p.k + 1) * L * p.N * ((B * B + 2) / 12.0) * tv +
         w2 * (1.0 + (double)p.k * p.N / 2.0) * std::ldexp(1.0, 2 * (64 - beta * L)) / 12.0;
}
int fhe_extprod_plan(const fhe_params* params, double w_norm2, int32_t* base_log, int32_t* level) {
  std::string why;
  if (validate(params, why)) return fail(nullptr, FHE_E_ARG, why);
  if (!(w_norm2 >= 0)) return fail(nullptr, FHE_E_ARG, "bad extprod-plan arguments (w_norm2 >= 0)");
  const fhe_params& p = *params;
  if (base_log) *base_log = 0;
  if (level) *level = 0;
  for (int L = 1; L <= 8; ++L)
    for (int beta = 7; beta >= 1; --beta)
      if (pack_gadget_ok(beta, L) &&
          std::ldexp(1.0, 63 - p.msg_bits) / std::sqrt(extprod_var(p, w_norm2, beta, L)) >= 9.2) {
        if (base_log) *base_log = beta;
        if (level) *level = L;
        return FHE_OK;
      }
  return fail(nullptr, FHE_E_STATE, "no ggsw gadget keeps 2^(63 - msg_bits) at 9.2 sigma for this query norm");
}

// Km: masks, Kn: noise (the full form passes its one key twice); body_only: the
// seeded form's output, (k+1) L x N body words
static int encrypt_ggsw_impl(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t beta, int32_t L, const ChaKey& Km,
                             const ChaKey& Kn, bool body_only, uint64_t id0, uint64_t* d_ggsw, void* stream) {
  int rc = ggsw_args(ctx, 0, D, beta, L);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if ((rc = need_secret(ctx))) return rc;
  if (!d_w || !d_ggsw) return fail(ctx, FHE_E_ARG, "null ggsw buffers");
  const fhe_params& p = ctx->p;
  hipLaunchKernelGGL(k_encrypt_ggsw, dim3((unsigned)((p.k + 1) * L)), dim3(256), 8 * (size_t)p.N + p.N,
                     (hipStream_t)stream, Km, Kn, p.N, p.k, (int)L, (int)beta, p.glwe_noise_bits, ctx->s_big, d_w,
                     (int)D, (u64)id0, d_ggsw, (int)body_only);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
int fhe_encrypt_ggsw(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t base_log, int32_t level, uint64_t seed,
                     uint64_t id0, uint64_t* d_ggsw, void* stream) {
  const ChaKey K = key_from_seed(seed);
  return encrypt_ggsw_impl(ctx, d_w, D, base_log, level, K, K, false, id0, d_ggsw, stream);
}
int fhe_encrypt_ggsw_key(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t base_log, int32_t level,
                         const uint32_t h_key[8], uint64_t id0, uint64_t* d_ggsw, void* stream) {
  ChaKey K;
  if (!key_arg(h_key, K)) return fail(ctx, FHE_E_ARG, "null encryption key");
  return encrypt_ggsw_impl(ctx, d_w, D, base_log, level, K, K, false, id0, d_ggsw, stream);
}

// documents per GLWE and GLWEs per batch
static int ggsw_slots(const fhe_params& p, int32_t D) { return p.N / D; }
static int64_t ggsw_glwes(const fhe_params& p, int64_t B, int32_t D) {
  const int S = ggsw_slots(p, D);
  return (B + S - 1) / S;
}
size_t fhe_glwe_docs_bytes(const fhe_params* p, int64_t B, int32_t D, int32_t level) {
  if (!p || B < 0 || D <= 0 || D > p->N || level < 1 || level > 8) return 0;
  return (size_t)((ggsw_glwes(*p, B, D) + 15) / 16) * 16 * (size_t)(p->k + 1) * p->N * level;
}
int fhe_glwe_docs_pack(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t B, int32_t D, int32_t base_log, int32_t level,
                       void* d_docs8, void* stream) {
  int rc = ggsw_args(ctx, B, D, base_log, level);  // argument errors first
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  if (B > 0 && (!d_glwe || !d_docs8)) return fail(ctx, FHE_E_ARG, "null ggsw document buffers");
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const int n1 = (p.k + 1) * p.N, KB = n1 * level / 64;
  const int64_t G = ggsw_glwes(p, B, D), ncb = (G + 15) / 16;
  if (ncb > 65535) return fail(ctx, FHE_E_ARG, "ggsw document batch too large: split the call");
  HIPCHK(ctx, hipMemsetAsync(d_docs8, 0, fhe_glwe_docs_bytes(&p, B, D, level), st));
  hipLaunchKernelGGL(k_glwe_digits, dim3((unsigned)(n1 / 64), (unsigned)ncb), dim3(256), 0, st, d_glwe, G, n1,
                     (int)base_log, (int)level, KB, (uint32_t*)d_docs8);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// planes -> GEMM -> slot extraction with cst on the body; the base log lives in
// the operands (the digits in d_docs8, the rows' scale). Workspace (context
// owned, allocated on first use): the query's Toeplitz byte planes
// (8 ((k+1)N)^2 L bytes) | zero bodies (G) | the GEMM's G x (k+1)N result.
static int linear_ggsw_impl(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t L, const void* d_docs8, int64_t B,
                            int32_t D, int64_t cst, uint64_t* d_out, hipStream_t st) {
  const fhe_params& p = ctx->p;
  const int n1 = (p.k + 1) * p.N, K = n1 * L, KB = K / 64, NB = n1 / 16, S = ggsw_slots(p, D);
  const int64_t G = ggsw_glwes(p, B, D);
  if (B > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "ggsw document batch too large: split the call");
  if (n1 % 64 || KB % KSM_RING) return fail(ctx, FHE_E_ARG, "ggsw product needs (k+1)N a multiple of 256");
  const size_t pbytes = (size_t)K * n1 * 8, bbytes = 8 * (size_t)G;
  const size_t need = pbytes + bbytes + 8 * (size_t)G * n1;
  int rc = reserve(ctx, ctx->xp_ws, need, FHE_E_DEVICE, "hipMalloc of the ggsw product workspace failed");
  if (rc) return rc;
  v4i* P8 = (v4i*)ctx->xp_ws.p;
  u64* body = (u64*)((char*)ctx->xp_ws.p + pbytes);
  u64* M = body + G;
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_xp, st, &e1);
  // the GEMM's K split (gemm81) adds its partial sums into the zeroed result
  HIPCHK(ctx, hipMemsetAsync(body, 0, bbytes + 8 * (size_t)G * n1, st));
  hipLaunchKernelGGL(k_extprod_planes, dim3((unsigned)(KB * NB)), dim3(64), 0, st, d_ggsw, p.N, p.k, (int)L, NB, P8);
  if ((rc = gemm81(ctx, ctx->prof_xp, "ggsw document", d_docs8, P8, body, G, n1, NB, KB, M, st))) return rc;
  hipLaunchKernelGGL(k_extprod_extract, dim3((unsigned)B, (unsigned)((p.k * p.N + 256) / 256)), dim3(256), 0, st, M,
                     S, (int)D, p.N, p.k, (u64)cst << (64 - p.msg_bits), d_out);
  prof_end(ctx, ctx->prof_xp, st, e1, B);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_linear_ggsw_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs8,
                          int64_t B, int32_t D, int64_t cst, uint64_t* d_out, void* stream) {
  int rc = ggsw_args(ctx, B, D, base_log, level);  // argument errors first
  if (rc) return rc;
  if ((rc = need_device(ctx))) return rc;
  if (B > 0 && (!d_ggsw || !d_docs8 || !d_out)) return fail(ctx, FHE_E_ARG, "null linear ggsw buffers");
  if (B == 0) return FHE_OK;
  return linear_ggsw_impl(ctx, d_ggsw, level, d_docs8, B, D, cst, d_out, (hipStream_t)stream);
}

int fhe_compare_ggsw_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs8,
                           int64_t B, int32_t D, int64_t cst, int64_t T, int64_t* d_acc, int64_t* d_below,
                           void* stream) {
  int rc = ggsw_args(ctx, B, D, base_log, level);  // argument errors first
  if (rc) return rc;
  if ((rc = need_secret(ctx))) return rc;
  if (B > 0 && (!d_ggsw || !d_docs8 || !d_acc || !d_below)) return fail(ctx, FHE_E_ARG, "null compare ggsw arguments");
  if (B == 0) return FHE_OK;
  QueryWs w;
  if ((rc = leveled_ws(ctx, B, 0, false, &w, nullptr))) return rc;
  rc = linear_ggsw_impl(ctx, d_ggsw, level, d_docs8, B, D, cst - T, w.ctv, (hipStream_t)stream);
  if (rc) return rc;
  return post_leveled_compare(ctx, w, B, T, d_acc, d_below, stream);
}

int fhe_search_ggsw_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs8,
                          int64_t B, int32_t D, int64_t cst, int64_t T, int32_t levels_bit, uint64_t* d_glwe_acc,
                          uint64_t* d_glwe_bit, void* stream) {
  int rc = ggsw_args(ctx, B, D, base_log, level);  // argument errors first
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8) return fail(ctx, FHE_E_ARG, "bad search ggsw arguments (levels_bit outside [0, 8])");
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if (levels_bit > ctx->pack_key.level) return fail(ctx, FHE_E_ARG, "search ggsw levels_bit exceeds the packing key's levels");
  if (B > 0 && (!d_ggsw || !d_docs8 || !d_glwe_acc || !d_glwe_bit))
    return fail(ctx, FHE_E_ARG, "null search ggsw arguments");
  if (B == 0) return FHE_OK;
  QueryWs w;
  if ((rc = leveled_ws(ctx, B, 0, true, &w, nullptr))) return rc;
  rc = linear_ggsw_impl(ctx, d_ggsw, level, d_docs8, B, D, cst - T, w.ctv, (hipStream_t)stream);
  if (rc) return rc;
  return post_leveled_search(ctx, w, B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}

// ---- both-private search: Q GGSW queries in one pass (k_extprod_q.h, §8.10) --
static int ggsws_args(fhe_ctx* ctx, int64_t Q, int64_t B, int32_t D, int32_t beta, int32_t L) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (Q < 1 || B < 1 || D <= 0) return fail(ctx, FHE_E_ARG, "bad ggsw queries arguments (Q < 1, B < 1 or D <= 0)");
  if (D > ctx->p.N) return fail(ctx, FHE_E_ARG, "ggsw queries dimension D > N: a document must fit one GLWE");
  // the query is a grid dimension of the extraction
  if (Q > 65535) return fail(ctx, FHE_E_ARG, "ggsw queries batch Q > 65535: split the call");
  if (B > 0x7fffffffLL || Q * B > 0x7fffffffLL)
    return fail(ctx, FHE_E_ARG, "ggsw queries result count too large (Q*B >= 2^31)");
  if (!pack_gadget_ok(beta, L))
    return fail(ctx, FHE_E_ARG, "ggsw queries gadget out of range (1 <= base_log <= 7, 1 <= level <= 8, "
                                "level * (base_log + 1) <= 62)");
  if (ctx->p.N % 256) return fail(ctx, FHE_E_ARG, "ggsw queries product needs N a multiple of 256");
  return FHE_OK;
}
size_t fhe_glwe_docs_queries_bytes(const fhe_params* p, int64_t B, int32_t D, int32_t level) {
  if (!p || B < 0 || D <= 0 || D > p->N || level < 1 || level > 8) return 0;
  return (size_t)ggsw_glwes(*p, B, D) * (size_t)(p->k + 1) * level * xq_fstride(p->N);
}
int fhe_glwe_docs_queries_pack(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t B, int32_t D, int32_t base_log,
                               int32_t level, void* d_docs, void* stream) {
  int rc = ggsws_args(ctx, 1, B, D, base_log, level);  // argument errors first
  if (rc) return rc;
  if (!d_glwe || !d_docs) return fail(ctx, FHE_E_ARG, "null ggsw queries document buffers");
  if ((rc = need_device(ctx))) return rc;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const int n1 = (p.k + 1) * p.N;
  const int64_t G = ggsw_glwes(p, B, D);
  if (G > 65535) return fail(ctx, FHE_E_ARG, "ggsw queries document batch too large: split the call");
  HIPCHK(ctx, hipMemsetAsync(d_docs, 0, fhe_glwe_docs_queries_bytes(&p, B, D, level), st));
  hipLaunchKernelGGL(k_glwe_digits_rev, dim3((unsigned)((n1 + 1023) / 1024), (unsigned)G), dim3(256), 0, st, d_glwe,
                     p.N, p.k, (int)base_log, (int)level, (uint8_t*)d_docs);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// row tiles of the GEMM (16 rows (q, c') each), padded to whole workgroup tiles
static int64_t ggsws_row_tiles(const fhe_params& p, int64_t Q, int* RT) {
  const int64_t rtn = (Q * (p.k + 1) + 15) / 16;
  *RT = rtn > 1 ? 2 : 1;
  return (rtn + *RT - 1) / *RT * *RT;
}
size_t fhe_ggsws_ws_bytes(const fhe_params* p, int64_t Q, int64_t B, int32_t D, int32_t level) {
  if (!p || Q < 1 || B < 1 || D <= 0 || D > p->N || level < 1 || level > 8) return 0;
  int RT;
  const size_t rtp = (size_t)ggsws_row_tiles(*p, Q, &RT);
  const size_t n1 = (size_t)(p->k + 1) * p->N, G = (size_t)ggsw_glwes(*p, B, D);
  // byte planes: 8 bytes per padded row and k | the result | the constants
  return rtp * 16 * n1 * level * 8 + 8 * (size_t)Q * G * n1 + 8 * (size_t)Q;
}

// planes -> GEMM -> slot extraction, h_cst[q] (or cst - h_T[q]) on query q's
// bodies, into d_out (Q B x (kN+1), query-major)
static int linear_ggsws_impl(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t L, const void* d_docs, int64_t Q,
                             int64_t B, int32_t D, const int64_t* h_cst, int64_t cst, const int64_t* h_T,
                             uint64_t* d_out, hipStream_t st) {
  const fhe_params& p = ctx->p;
  const int n1 = (p.k + 1) * p.N, KB = n1 * L / 64, S = ggsw_slots(p, D);
  const int64_t G = ggsw_glwes(p, B, D);
  int RT;
  const int64_t rtp = ggsws_row_tiles(p, Q, &RT), rgrid = rtp / RT;
  const int64_t cgrid = G * (p.N / 16) / XQ_CG;  // N % 256 == 0: whole workgroups
  if (G > 65535 || rgrid > 65535 || cgrid > 0x7fffffffLL)
    return fail(ctx, FHE_E_ARG, "ggsw queries batch too large: split the call");
  const size_t need = fhe_ggsws_ws_bytes(&p, Q, B, D, L);
  int rc = reserve(ctx, ctx->xp_ws, need, FHE_E_DEVICE, "hipMalloc of the ggsw product workspace failed");
  if (rc) return rc;
  const size_t pbytes = (size_t)rtp * 16 * n1 * L * 8, mbytes = 8 * (size_t)Q * G * n1;
  v4i* P8 = (v4i*)ctx->xp_ws.p;
  u64* M = (u64*)((char*)ctx->xp_ws.p + pbytes);
  u64* d_cst = M + (size_t)Q * G * n1;
  if ((rc = store_scaled_csts(ctx, d_cst, Q, h_cst, cst, h_T, st))) return rc;
  const auto [Sk, kslice] = xq_ksplit(KB, cgrid * rgrid);
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_xq, st, &e1);
  ctx->prof_xq.kernel = RT == 2 ? "k_extprod_queries_mfma<2>" : "k_extprod_queries_mfma<1>";
  if (Sk > 1) HIPCHK(ctx, hipMemsetAsync(M, 0, mbytes, st));
  hipLaunchKernelGGL(k_ggsws_planes, dim3((unsigned)KB, (unsigned)rtp), dim3(64), 0, st, d_ggsw, p.N, p.k, (int)L,
                     (int)Q, P8);
  const dim3 grid((unsigned)cgrid, (unsigned)rgrid, (unsigned)Sk);
  xq_dispatch(RT, [&, kslice = kslice](auto rt) {
    hipLaunchKernelGGL(k_extprod_queries_mfma<decltype(rt)::value>, grid, dim3(256), 0, st, (const v4i*)P8,
                       (const uint8_t*)d_docs, p.N, p.k, (int)L, (int)Q, (int)G, KB, kslice, M);
  });
  hipLaunchKernelGGL(k_extprod_extract_queries, dim3((unsigned)B, (unsigned)((p.k * p.N + 256) / 256), (unsigned)Q),
                     dim3(256), 0, st, M, S, (int)D, p.N, p.k, G, B, d_cst, d_out);
  prof_end(ctx, ctx->prof_xq, st, e1, Q * B);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_linear_ggsws_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs,
                           int64_t Q, int64_t B, int32_t D, const int64_t* h_cst, uint64_t* d_out, void* stream) {
  int rc = ggsws_args(ctx, Q, B, D, base_log, level);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (!d_ggsw || !d_docs || !h_cst || !d_out) return fail(ctx, FHE_E_ARG, "null linear ggsw queries arguments");
  if ((rc = need_device(ctx))) return rc;
  return linear_ggsws_impl(ctx, d_ggsw, level, d_docs, Q, B, D, h_cst, 0, nullptr, d_out, (hipStream_t)stream);
}

// the leveled workspace for Q B results with the Q thresholds in the query's place
static int ggsws_leveled(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t L, const void* d_docs, int64_t Q, int64_t B,
                         int32_t D, int64_t cst, const int64_t* h_T, bool keep_copy, QueryWs* w, int64_t** d_T,
                         void* stream) {
  hipStream_t st = (hipStream_t)stream;
  u64* ex;
  int rc = leveled_ws(ctx, Q * B, (size_t)Q, keep_copy, w, &ex);
  if (rc) return rc;
  *d_T = (int64_t*)ex;
  if ((rc = store_words(ctx, ex, (const u64*)h_T, Q, st))) return rc;
  return linear_ggsws_impl(ctx, d_ggsw, L, d_docs, Q, B, D, nullptr, cst, h_T, w->ctv, st);
}

int fhe_compare_ggsws_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs,
                            int64_t Q, int64_t B, int32_t D, int64_t cst, const int64_t* h_T, int64_t* d_acc,
                            int64_t* d_below, void* stream) {
  int rc = ggsws_args(ctx, Q, B, D, base_log, level);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (!d_ggsw || !d_docs || !h_T || !d_acc || !d_below)
    return fail(ctx, FHE_E_ARG, "null compare ggsw queries arguments");
  if ((rc = need_secret(ctx))) return rc;
  QueryWs w;
  int64_t* d_T;
  rc = ggsws_leveled(ctx, d_ggsw, level, d_docs, Q, B, D, cst, h_T, false, &w, &d_T, stream);
  if (rc) return rc;
  return post_leveled_compare_queries(ctx, w, Q, B, d_T, d_acc, d_below, stream);
}

int fhe_search_ggsws_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs,
                           int64_t Q, int64_t B, int32_t D, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                           uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream) {
  int rc = ggsws_args(ctx, Q, B, D, base_log, level);  // argument errors first: a host-only context reports them too
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad search ggsw queries arguments (levels_bit outside [0, 8])");
  if (!d_ggsw || !d_docs || !h_T || !d_glwe_acc || !d_glwe_bit)
    return fail(ctx, FHE_E_ARG, "null search ggsw queries arguments");
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if (levels_bit > ctx->pack_key.level)
    return fail(ctx, FHE_E_ARG, "search ggsw queries levels_bit exceeds the packing key's levels");
  QueryWs w;
  int64_t* d_T;
  rc = ggsws_leveled(ctx, d_ggsw, level, d_docs, Q, B, D, cst, h_T, true, &w, &d_T, stream);
  if (rc) return rc;
  // result q B + b is ciphertext q B + b of the batch: coefficient (q B + b) mod N
  // of GLWE (q B + b) / N
  return post_leveled_search(ctx, w, Q * B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}

// ---- both-private search on seeded payloads (k_private_seeded.h, §8.15) -----
size_t fhe_ggsw_body_words(const fhe_params* p, int32_t base_log, int32_t level) {
  if (!p || !pack_gadget_ok(base_log, level)) return 0;
  return (size_t)(p->k + 1) * level * p->N;
}
// an argument error of a full-form sibling's checks, told as a seeded entry's
static int seeded_arg(fhe_ctx* ctx, int rc) {
  if (rc != FHE_E_ARG) return rc;
  return fail(ctx, FHE_E_ARG, std::string("seeded: ") + fhe_last_error(ctx));
}

int fhe_encrypt_packed_seeded_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D,
                                    const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], uint64_t id0,
                                    uint64_t* d_body, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  ChaKey Km, Kn;  // argument errors first: a host-only context reports them too
  if (!key_arg(h_mask_key, Km) || !key_arg(h_noise_key, Kn))
    return fail(ctx, FHE_E_ARG, "seeded packed-encrypt: null mask or noise key");
  if (B < 0 || D <= 0 || (B > 0 && (!d_qx || !d_body)))
    return fail(ctx, FHE_E_ARG, "bad seeded packed-encrypt arguments");
  return seeded_arg(ctx, encrypt_packed_impl(ctx, d_qx, B, D, Km, Kn, true, id0, d_body, stream));
}

int fhe_encrypt_ggsw_seeded(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t base_log, int32_t level,
                            const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], uint64_t id0,
                            uint64_t* d_body, void* stream) {
  int rc = seeded_arg(ctx, ggsw_args(ctx, 0, D, base_log, level));  // argument errors first
  if (rc) return rc;
  ChaKey Km, Kn;
  if (!key_arg(h_mask_key, Km) || !key_arg(h_noise_key, Kn))
    return fail(ctx, FHE_E_ARG, "seeded ggsw: null mask or noise key");
  if (!d_w || !d_body) return fail(ctx, FHE_E_ARG, "null seeded ggsw buffers");
  return seeded_arg(ctx, encrypt_ggsw_impl(ctx, d_w, D, base_log, level, Km, Kn, true, id0, d_body, stream));
}

// rows x N bodies -> rows x (k+1)N full form (k_expand_ggsw_seeded's addressing)
static int expand_private_impl(fhe_ctx* ctx, const ChaKey& Km, uint32_t tag, const uint64_t* d_body,
                               const uint64_t* d_ids, uint64_t id_base, int64_t items, int64_t rows, int row_ids,
                               int comp_ids, int comp_blk, uint64_t* d_out, hipStream_t st) {
  const fhe_params& p = ctx->p;
  if (items * rows > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "seeded expansion too large: split the call");
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_xs, st, &e1);
  ctx->prof_xs.kernel = "k_expand_ggsw_seeded";
  hipLaunchKernelGGL(k_expand_ggsw_seeded, dim3((unsigned)(items * rows)), dim3(256), 0, st, Km, tag, d_body, d_ids,
                     (u64)id_base, rows, row_ids, comp_ids, comp_blk, p.N, p.k, d_out);
  prof_end(ctx, ctx->prof_xs, st, e1, items);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_expand_packed_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int64_t B, int32_t D,
                                   const uint32_t h_mask_key[8], uint64_t* d_glwe, void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  ChaKey Km;  // argument errors first: a host-only context reports them too
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded packed expansion: null mask key");
  if (B < 0 || D <= 0 || (B > 0 && (!d_body || !d_glwe)))
    return fail(ctx, FHE_E_ARG, "bad seeded packed expansion arguments");
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  const int64_t G = packed_chunks(p, D);
  if (B * G > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "seeded packed expansion too large: split the call");
  return expand_private_impl(ctx, Km, TAG_ENC_MASK, d_body, nullptr, id0, 1, B * G, 1, 0, p.N / 8, d_glwe,
                             (hipStream_t)stream);
}

// Q queries' bodies -> Q GGSWs; the stream ids from d_ids (Q of them, device) or, for one query, id_base
static int expand_ggsws_impl(fhe_ctx* ctx, const ChaKey& Km, const uint64_t* d_body, const uint64_t* d_ids,
                             uint64_t id_base, int64_t Q, int32_t L, uint64_t* d_ggsw, hipStream_t st) {
  const fhe_params& p = ctx->p;
  return expand_private_impl(ctx, Km, TAG_GGSW_MASK, d_body, d_ids, id_base, Q, (int64_t)(p.k + 1) * L, p.k, 1, 0,
                             d_ggsw, st);
}

int fhe_expand_ggsws_seeded(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t Q, int32_t base_log,
                            int32_t level, const uint32_t h_mask_key[8], uint64_t* d_ggsw, void* stream) {
  int rc = seeded_arg(ctx, ggsw_args(ctx, 0, 1, base_log, level));  // argument errors first
  if (rc) return rc;
  ChaKey Km;
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded ggsw expansion: null mask key");
  if (Q < 1 || Q > 65535) return fail(ctx, FHE_E_ARG, "bad seeded ggsw expansion arguments (Q outside [1, 65535])");
  if (!d_body || !d_id0 || !d_ggsw) return fail(ctx, FHE_E_ARG, "null seeded ggsw expansion buffers");
  if ((rc = need_device(ctx))) return rc;
  return expand_ggsws_impl(ctx, Km, d_body, d_id0, 0, Q, level, d_ggsw, (hipStream_t)stream);
}

int fhe_glwe_docs_pack_seeded(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int64_t B, int32_t D,
                              int32_t base_log, int32_t level, const uint32_t h_mask_key[8], void* d_docs8,
                              void* stream) {
  int rc = seeded_arg(ctx, ggsw_args(ctx, B, D, base_log, level));  // argument errors first
  if (rc) return rc;
  ChaKey Km;
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded ggsw documents: null mask key");
  if (B > 0 && (!d_body || !d_docs8)) return fail(ctx, FHE_E_ARG, "null seeded ggsw document buffers");
  const fhe_params& p = ctx->p;
  const int n1 = (p.k + 1) * p.N, KB = n1 * level / 64;
  if (n1 % 128) return fail(ctx, FHE_E_ARG, "seeded ggsw documents need (k+1)N a multiple of 128");
  const int64_t G = ggsw_glwes(p, B, D), ncb = (G + 15) / 16;
  if (ncb > 65535) return fail(ctx, FHE_E_ARG, "seeded ggsw document batch too large: split the call");
  if ((rc = need_device(ctx))) return rc;
  if (B == 0) return FHE_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(ctx, hipMemsetAsync(d_docs8, 0, fhe_glwe_docs_bytes(&p, B, D, level), st));
  hipLaunchKernelGGL(k_glwe_digits_seeded, dim3((unsigned)(n1 / 128), (unsigned)ncb), dim3(256), 0, st, Km, d_body,
                     (u64)id0, G, p.N, p.k, (int)base_log, (int)level, KB, (uint32_t*)d_docs8);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_glwe_docs_queries_pack_seeded(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int64_t B, int32_t D,
                                      int32_t base_log, int32_t level, const uint32_t h_mask_key[8], void* d_docs,
                                      void* stream) {
  int rc = seeded_arg(ctx, ggsws_args(ctx, 1, B, D, base_log, level));  // argument errors first
  if (rc) return rc;
  ChaKey Km;
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded ggsw queries documents: null mask key");
  if (!d_body || !d_docs) return fail(ctx, FHE_E_ARG, "null seeded ggsw queries document buffers");
  const fhe_params& p = ctx->p;
  const int n1 = (p.k + 1) * p.N;
  const int64_t G = ggsw_glwes(p, B, D);
  if (G > 65535) return fail(ctx, FHE_E_ARG, "seeded ggsw queries document batch too large: split the call");
  if ((rc = need_device(ctx))) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(ctx, hipMemsetAsync(d_docs, 0, fhe_glwe_docs_queries_bytes(&p, B, D, level), st));
  hipLaunchKernelGGL(k_glwe_digits_rev_seeded, dim3((unsigned)((n1 + 2047) / 2048), (unsigned)G), dim3(256), 0, st, Km,
                     d_body, (u64)id0, p.N, p.k, (int)base_log, (int)level, (uint8_t*)d_docs);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

// the search entries on seeded queries: expand into the context's workspace,
// then the full-form entry, whose checks ran here first (no work is queued
// for a call that fails)
static int search_seeded_keys(fhe_ctx* ctx, int32_t levels_bit) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if (levels_bit > ctx->pack_key.level)
    return fail(ctx, FHE_E_ARG, "seeded search ggsw levels_bit exceeds the packing key's levels");
  return FHE_OK;
}
static int expand_queries_ws(fhe_ctx* ctx, const ChaKey& Km, const uint64_t* d_body, const uint64_t* d_ids,
                             uint64_t id_base, int64_t Q, int32_t base_log, int32_t level, void* stream) {
  const size_t need = 8 * (size_t)Q * fhe_ggsw_words(&ctx->p, base_log, level);
  int rc = reserve(ctx, ctx->xs_ws, need, FHE_E_DEVICE, "hipMalloc of the seeded ggsw expansion workspace failed");
  if (rc) return rc;
  return expand_ggsws_impl(ctx, Km, d_body, d_ids, id_base, Q, level, (uint64_t*)ctx->xs_ws.p, (hipStream_t)stream);
}

int fhe_search_ggsw_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int32_t base_log, int32_t level,
                                 const uint32_t h_mask_key[8], const void* d_docs8, int64_t B, int32_t D, int64_t cst,
                                 int64_t T, int32_t levels_bit, uint64_t* d_glwe_acc, uint64_t* d_glwe_bit,
                                 void* stream) {
  int rc = seeded_arg(ctx, ggsw_args(ctx, B, D, base_log, level));  // argument errors first
  if (rc) return rc;
  ChaKey Km;
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded search ggsw: null mask key");
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad seeded search ggsw arguments (levels_bit outside [0, 8])");
  if (B > 0 && (!d_body || !d_docs8 || !d_glwe_acc || !d_glwe_bit))
    return fail(ctx, FHE_E_ARG, "null seeded search ggsw arguments");
  if ((rc = search_seeded_keys(ctx, levels_bit))) return rc;
  if (B == 0) return FHE_OK;
  if ((rc = expand_queries_ws(ctx, Km, d_body, nullptr, id0, 1, base_log, level, stream))) return rc;
  return seeded_arg(ctx, fhe_search_ggsw_batch(ctx, (const uint64_t*)ctx->xs_ws.p, base_log, level, d_docs8, B, D, cst,
                                               T, levels_bit, d_glwe_acc, d_glwe_bit, stream));
}

int fhe_search_ggsws_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int32_t base_log,
                                  int32_t level, const uint32_t h_mask_key[8], const void* d_docs, int64_t Q,
                                  int64_t B, int32_t D, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                                  uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream) {
  int rc = seeded_arg(ctx, ggsws_args(ctx, Q, B, D, base_log, level));  // argument errors first
  if (rc) return rc;
  ChaKey Km;
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded search ggsw queries: null mask key");
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad seeded search ggsw queries arguments (levels_bit outside [0, 8])");
  if (!d_body || !d_id0 || !d_docs || !h_T || !d_glwe_acc || !d_glwe_bit)
    return fail(ctx, FHE_E_ARG, "null seeded search ggsw queries arguments");
  if ((rc = search_seeded_keys(ctx, levels_bit))) return rc;
  if ((rc = expand_queries_ws(ctx, Km, d_body, d_id0, 0, Q, base_log, level, stream))) return rc;
  return seeded_arg(ctx, fhe_search_ggsws_batch(ctx, (const uint64_t*)ctx->xs_ws.p, base_log, level, d_docs, Q, B, D,
                                                cst, h_T, levels_bit, d_glwe_acc, d_glwe_bit, stream));
}

// ---- seeded evaluation keys (k_seeded_keys.h) -------------
// A key travels as its rows' bodies and the public mask key its masks came
// from. One mask key serves one generated key: the main set (distinct tags)
// shares one, the packing key and the bridge key have their own.
size_t fhe_bsk_body_words(const fhe_params* p) {
  return p ? (size_t)p->n * (p->k + 1) * p->pbs_level * p->N : 0;
}
size_t fhe_ksk_body_words(const fhe_params* p) { return p ? (size_t)p->k * p->N * p->ks_level : 0; }
size_t fhe_fast_bsk_body_words(const fhe_params* p, int32_t which) {
  return p ? fhe_fast_bsk_words(p, which) / (size_t)(p->k + 1) : 0;
}
size_t fhe_pack_key_body_words(const fhe_params* p, int32_t base_log, int32_t level) {
  if (!p || !pack_gadget_ok(base_log, level)) return 0;
  return PACK_KEY.body_words(*p, level);
}
size_t fhe_bridge_key_body_words(const fhe_params* p, int32_t base_log, int32_t level) {
  if (!p || !pack_gadget_ok(base_log, level)) return 0;
  return BRIDGE_KEY.body_words(*p, level);
}

// One key as rows: `rows` rows of n1 words in `key`, the last `body` words of a
// row its body (N: a GLWE row, masks from streams (tag, r k + c); 1: an LWE
// row, masks from stream (tag, r)).
struct KeyRows {
  u64* key;
  int64_t rows;
  int n1, body;
  uint32_t tag;
};
static KeyRows bsk_rows(const fhe_ctx* ctx, int g) {  // g = 0: the main key
  const fhe_params& p = ctx->p;
  const int n1 = (p.k + 1) * p.N;
  if (g == 0) return {ctx->bsk, (int64_t)p.n * (p.k + 1) * p.pbs_level, n1, p.N, TAG_BSK_MASK};
  return {ctx->bskf[g - 1], (int64_t)fast_ggsws(p, g) * (p.k + 1) * fast_level(p, g), n1, p.N,
          mb_for(p, g) ? kTagMbMask[g] : kTagMask[g]};
}
static KeyRows ksk_rows(const fhe_ctx* ctx) {
  const fhe_params& p = ctx->p;
  return {ctx->ksk, (int64_t)p.k * p.N * p.ks_level, p.n + 1, 1, TAG_KSK_MASK};
}
static KeyRows gadget_rows(fhe_ctx* ctx, const GadgetDesc& d, int L) {
  const fhe_params& p = ctx->p;
  return {d.key(ctx).key, (int64_t)p.k * p.N * L, d.n1(p), d.body(p), d.tag_mask};
}
static int sk_reserve(fhe_ctx* ctx, size_t words) {
  return reserve(ctx, ctx->sk_ws, 8 * words, FHE_E_DEVICE, "hipMalloc of the seeded keys' staging buffer failed");
}
static int sk_release(fhe_ctx* ctx) {
  if (ctx->sk_ws.p) {
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipFree(ctx->sk_ws.p));
    ctx->sk_ws = DevBuf{};
  }
  return FHE_OK;
}
// the key's bodies, packed, to the host
static int export_bodies(fhe_ctx* ctx, const KeyRows& r, uint64_t* h_out) {
  const int64_t words = r.rows * r.body;
  int rc = sk_reserve(ctx, (size_t)words);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gather_key_bodies, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, nullptr, r.key, r.rows,
                     r.n1, r.n1 - r.body, r.body, (u64*)ctx->sk_ws.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpy(h_out, ctx->sk_ws.p, 8 * (size_t)words, hipMemcpyDeviceToHost));
  return FHE_OK;
}
// bodies from the host -> the key in standard form, its masks regenerated under Km
static int import_bodies(fhe_ctx* ctx, const ChaKey& Km, const KeyRows& r, const uint64_t* h_in) {
  const fhe_params& p = ctx->p;
  const int64_t words = r.rows * r.body;
  int rc = sk_reserve(ctx, (size_t)words);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpy(ctx->sk_ws.p, h_in, 8 * (size_t)words, hipMemcpyHostToDevice));
  if (r.body == 1) {
    const int64_t blocks = r.rows * ((r.n1 - 1 + 7) / 8);
    hipLaunchKernelGGL(k_expand_lwe_rows_seeded, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, nullptr, Km,
                       r.tag, (const u64*)ctx->sk_ws.p, r.rows, r.n1, r.key);
  } else {
    hipLaunchKernelGGL(k_expand_ggsw_seeded, dim3((unsigned)r.rows), dim3(256), 0, nullptr, Km, r.tag,
                       (const u64*)ctx->sk_ws.p, (const u64*)nullptr, (u64)0, r.rows, p.k, 1, 0, p.N, p.k, r.key);
  }
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
static bool mask_used(const fhe_ctx* ctx, const ChaKey& K) {
  for (const ChaKey& u : ctx->used_masks)
    if (!memcmp(u.w, K.w, 32)) return true;
  return false;
}
static void note_mask(fhe_ctx* ctx, const ChaKey& K) {
  if (!mask_used(ctx, K)) ctx->used_masks.push_back(K);
}
static int mask_reuse(fhe_ctx* ctx, const GadgetDesc& d, const ChaKey& Km) {
  if (!mask_used(ctx, Km)) return FHE_OK;
  return fail(ctx, FHE_E_ARG, "seeded " + std::string(d.noun) + " keygen: mask key reuse: a seeded keygen of this context "
                              "already used this mask key (one mask key serves one generated key)");
}

int fhe_keygen_seeded(fhe_ctx* ctx, const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  ChaKey Km, Kn;  // argument errors first: a host-only context reports them too
  if (!key_arg(h_mask_key, Km) || !key_arg(h_noise_key, Kn))
    return fail(ctx, FHE_E_ARG, "seeded keygen: null mask or noise key");
  int rc = need_device(ctx);
  if (rc) return rc;
  if ((rc = keygen_impl(ctx, Km, Kn, (hipStream_t)stream, 1))) return rc;
  ctx->eval_seeded = ctx->fast_seeded = true;
  ctx->eval_mask = Km;
  note_mask(ctx, Km);
  return FHE_OK;
}

int fhe_keygen_pack_key_seeded(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_mask_key[8],
                               const uint32_t h_noise_key[8], void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = seeded_arg(ctx, gadget_args(ctx, PACK_KEY, base_log, level));
  if (rc) return rc;
  ChaKey Km, Kn;
  if (!key_arg(h_mask_key, Km) || !key_arg(h_noise_key, Kn))
    return fail(ctx, FHE_E_ARG, "seeded packing keygen: null mask or noise key");
  if ((rc = mask_reuse(ctx, PACK_KEY, Km))) return rc;
  if ((rc = need_secret(ctx))) return rc;
  if ((rc = keygen_pack_impl(ctx, base_log, level, Km, Kn, (hipStream_t)stream))) return rc;
  ctx->pack_key.seeded = true;
  ctx->pack_key.mask = Km;
  note_mask(ctx, Km);
  return FHE_OK;
}

// the seeded bridge keygen of a slot; the mask key reuse refusal covers every
// slot of the context (used_masks is the context's)
static int keygen_bridge_key_seeded_at(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                                       int32_t level, const uint32_t h_mask_key[8], const uint32_t h_noise_key[8],
                                       void* stream) {
  int rc = seeded_arg(ctx, gadget_args(ctx, BRIDGE_KEY, base_log, level));
  if (rc) return rc;
  ChaKey Km, Kn;
  const bool keys_ok = key_arg(h_mask_key, Km) && key_arg(h_noise_key, Kn);
  if ((rc = bridge_keygen_args(ctx, h_s_big_old, keys_ok, "seeded: "))) return rc;
  if ((rc = mask_reuse(ctx, BRIDGE_KEY, Km))) return rc;
  if ((rc = need_secret(ctx))) return rc;
  if ((rc = keygen_bridge_impl(ctx, slot, h_s_big_old, base_log, level, Km, Kn, (hipStream_t)stream))) return rc;
  ctx->bridge_keys[slot].seeded = true;
  ctx->bridge_keys[slot].mask = Km;
  note_mask(ctx, Km);
  return FHE_OK;
}
int fhe_keygen_bridge_key_seeded(fhe_ctx* ctx, const uint64_t* h_s_big_old, int32_t base_log, int32_t level,
                                 const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  return keygen_bridge_key_seeded_at(ctx, 0, h_s_big_old, base_log, level, h_mask_key, h_noise_key, stream);
}
int fhe_keygen_bridge_key_slot_seeded(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                                      int32_t level, const uint32_t h_mask_key[8], const uint32_t h_noise_key[8],
                                      void* stream) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  return keygen_bridge_key_seeded_at(ctx, slot, h_s_big_old, base_log, level, h_mask_key, h_noise_key, stream);
}

int fhe_export_eval_keys_seeded(fhe_ctx* ctx, uint32_t h_mask_key_out[8], uint64_t* h_bsk_body, uint64_t* h_ksk_body,
                                uint64_t* const h_gadget_body[5]) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (!h_mask_key_out || !h_bsk_body || !h_ksk_body)
    return fail(ctx, FHE_E_ARG, "seeded export: the mask key, bsk body and ksk body buffers are required");
  const fhe_params& p = ctx->p;
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g) && (!h_gadget_body || !h_gadget_body[g - 1]))
      return fail(ctx, FHE_E_ARG, "seeded export: missing body buffer of gadget " + std::to_string(g) +
                                      " (these parameters have it)");
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  bool fast = false;
  for (int g = 1; g < NGAD; ++g) fast = fast || fast_level(p, g);
  if (!ctx->eval_seeded || (fast && !ctx->fast_seeded))
    return fail(ctx, FHE_E_STATE, !ctx->eval_seeded
                                      ? "these evaluation keys were not generated or imported seeded: no mask key "
                                        "(fhe_keygen_seeded, fhe_import_eval_keys_seeded)"
                                      : "the fast gadgets' keys were re-encrypted under a private key and cannot be "
                                        "exported seeded");
  HIPCHK(ctx, hipDeviceSynchronize());
  if ((rc = export_bodies(ctx, bsk_rows(ctx, 0), h_bsk_body))) return rc;
  if ((rc = export_bodies(ctx, ksk_rows(ctx), h_ksk_body))) return rc;
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g) && (rc = export_bodies(ctx, bsk_rows(ctx, g), h_gadget_body[g - 1]))) return rc;
  memcpy(h_mask_key_out, ctx->eval_mask.w, 32);
  return sk_release(ctx);
}

// Evaluation keys only, as fhe_import_eval_keys: no secret is ever allocated,
// and secrets already present are zeroed and freed.
int fhe_import_eval_keys_seeded(fhe_ctx* ctx, const uint32_t h_mask_key[8], const uint64_t* h_bsk_body,
                                const uint64_t* h_ksk_body, const uint64_t* const h_gadget_body[5]) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  ChaKey Km;  // argument errors first: a host-only context reports them too
  if (!key_arg(h_mask_key, Km)) return fail(ctx, FHE_E_ARG, "seeded import: null mask key");
  if (!h_bsk_body || !h_ksk_body)
    return fail(ctx, FHE_E_ARG, "seeded import: the bsk body and ksk body buffers are required");
  const fhe_params& p = ctx->p;
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g) && (!h_gadget_body || !h_gadget_body[g - 1]))
      return fail(ctx, FHE_E_ARG, "seeded import: missing key body of gadget " + std::to_string(g) +
                                      " (these parameters have it)");
  int rc = need_device(ctx);
  if (rc) return rc;
  if ((rc = drop_secrets(ctx))) return rc;
  if ((rc = alloc_keys(ctx, false))) return rc;
  ctx->eval_seeded = ctx->fast_seeded = false;
  if ((rc = import_bodies(ctx, Km, bsk_rows(ctx, 0), h_bsk_body))) return rc;
  if ((rc = import_bodies(ctx, Km, ksk_rows(ctx), h_ksk_body))) return rc;
  for (int g = 1; g < NGAD; ++g)
    if (fast_level(p, g) && (rc = import_bodies(ctx, Km, bsk_rows(ctx, g), h_gadget_body[g - 1]))) return rc;
  if ((rc = convert_bsk(ctx, nullptr))) return rc;
  if ((rc = sk_release(ctx))) return rc;  // synchronises
  ctx->keys = true;
  ctx->eval_seeded = ctx->fast_seeded = true;
  ctx->eval_mask = Km;
  return FHE_OK;
}

// the two gadget keys' seeded export and import, shared through GadgetDesc
static int gadget_key_export_seeded(fhe_ctx* ctx, const GadgetDesc& d, uint32_t* h_mask_key_out, uint64_t* h_body) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (!h_mask_key_out || !h_body)
    return fail(ctx, FHE_E_ARG, "seeded " + std::string(d.noun) + " key export: null buffer");
  int rc = need_gadget_key(ctx, d);
  if (rc) return rc;
  const GadgetKey& k = d.key(ctx);
  if (!k.seeded)
    return fail(ctx, FHE_E_STATE, "the " + std::string(d.noun) + " key was not generated or imported seeded: no mask "
                                  "key (fhe_keygen_" + d.abi + "_key_seeded, fhe_import_" + d.abi + "_key_seeded)");
  HIPCHK(ctx, hipDeviceSynchronize());
  if ((rc = export_bodies(ctx, gadget_rows(ctx, d, k.level), h_body))) return rc;
  memcpy(h_mask_key_out, k.mask.w, 32);
  return sk_release(ctx);
}
static int gadget_key_import_seeded(fhe_ctx* ctx, const GadgetDesc& d, int32_t beta, int32_t L,
                                    const uint32_t* h_mask_key, const uint64_t* h_body) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = seeded_arg(ctx, gadget_args(ctx, d, beta, L));  // argument errors first
  if (rc) return rc;
  ChaKey Km;
  if (!key_arg(h_mask_key, Km) || !h_body)
    return fail(ctx, FHE_E_ARG, "seeded " + std::string(d.noun) + " key import: null mask key or body buffer");
  if ((rc = need_device(ctx))) return rc;
  if ((rc = gadget_key_alloc(ctx, d, L))) return rc;
  if ((rc = import_bodies(ctx, Km, gadget_rows(ctx, d, L), h_body))) return rc;
  if ((rc = gadget_key_planes(ctx, d, beta, L, nullptr))) return rc;
  GadgetKey& k = d.key(ctx);
  k.seeded = true;
  k.mask = Km;
  return sk_release(ctx);
}
int fhe_export_pack_key_seeded(fhe_ctx* ctx, uint32_t h_mask_key_out[8], uint64_t* h_body) {
  return gadget_key_export_seeded(ctx, PACK_KEY, h_mask_key_out, h_body);
}
int fhe_export_bridge_key_seeded(fhe_ctx* ctx, uint32_t h_mask_key_out[8], uint64_t* h_body) {
  return gadget_key_export_seeded(ctx, BRIDGE_KEY, h_mask_key_out, h_body);
}
int fhe_export_bridge_key_slot_seeded(fhe_ctx* ctx, int32_t slot, uint32_t h_mask_key_out[8], uint64_t* h_body) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  return gadget_key_export_seeded(ctx, bridge_slot(slot), h_mask_key_out, h_body);
}
int fhe_import_bridge_key_slot_seeded(fhe_ctx* ctx, int32_t slot, int32_t base_log, int32_t level,
                                      const uint32_t h_mask_key[8], const uint64_t* h_body) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  int rc = slot_arg(ctx, slot);
  if (rc) return rc;
  return gadget_key_import_seeded(ctx, bridge_slot(slot), base_log, level, h_mask_key, h_body);
}
int fhe_import_pack_key_seeded(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_mask_key[8],
                               const uint64_t* h_body) {
  return gadget_key_import_seeded(ctx, PACK_KEY, base_log, level, h_mask_key, h_body);
}
int fhe_import_bridge_key_seeded(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_mask_key[8],
                                 const uint64_t* h_body) {
  return gadget_key_import_seeded(ctx, BRIDGE_KEY, base_log, level, h_mask_key, h_body);
}

int fhe_threshold_batch(fhe_ctx* ctx, const uint64_t* d_ct_acc, int64_t count, int64_t T, uint64_t* d_bit,
                        void* stream) {
  int rc = need_eval_keys(ctx);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!d_ct_acc || !d_bit))) return fail(ctx, FHE_E_ARG, "bad threshold arguments");
  if (count == 0) return FHE_OK;
  const fhe_params& p = ctx->p;
  hipStream_t st = (hipStream_t)stream;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
  // workspace: v = acc - T (B big, consumed by the extraction) | small (B)
  rc = ensure_ws(ctx, 8 * ((size_t)count * Wb + (size_t)count * Ws));
  if (rc) return rc;
  u64* ctv = (u64*)ctx->ws.p;
  u64* small = ctv + (size_t)count * Wb;
  const int64_t words = count * (int64_t)Wb;
  hipLaunchKernelGGL(k_lwe_affine, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, d_ct_acc, count, (int)Wb,
                     (u64)1, (u64)0 - ((u64)T << (64 - p.msg_bits)), ctv);
  HIPCHK(ctx, hipGetLastError());
  rc = sign_extract_batch(ctx, ctv, count, d_bit, small, st);
  if (rc) return rc;
  // [acc >= T] = 1 - [v < 0]: negate the sign ciphertext and add 2^63 to its body
  hipLaunchKernelGGL(k_lwe_affine, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, d_bit, count, (int)Wb,
                     (u64)0 - 1, 1ull << 63, d_bit);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

void fhe_key_from_seed(uint64_t seed, uint32_t h_key_out[8]) {
  const ChaKey K = key_from_seed(seed);
  for (int i = 0; i < 8; ++i) h_key_out[i] = K.w[i];
}

int fhe_quantize_pairs(fhe_ctx* ctx, const void* d_query, int32_t query_is_f64, const void* d_docs,
                       int32_t docs_is_f64, int64_t B, int32_t D, double scale, int64_t zero_point, int64_t qmin,
                       int64_t qmax, int64_t* d_qx, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B < 0 || D <= 0 || (B > 0 && (!d_docs || !d_qx)) || !(scale > 0) || qmin > qmax)
    return fail(ctx, FHE_E_ARG, "bad quantize arguments");
  if (B == 0) return FHE_OK;
  const int64_t total = B * D;
  const dim3 g((unsigned)((total + 255) / 256)), b(256);
  hipStream_t st = (hipStream_t)stream;
  const double z = (double)zero_point, lo = (double)qmin, hi = (double)qmax;
#define QLAUNCH(QT, DT) \
  hipLaunchKernelGGL((k_pair_quantize<QT, DT>), g, b, 0, st, (const QT*)d_query, (const DT*)d_docs, B, D, scale, z, lo, hi, d_qx)
  if (query_is_f64 && docs_is_f64) QLAUNCH(double, double);
  else if (query_is_f64) QLAUNCH(double, float);
  else if (docs_is_f64) QLAUNCH(float, double);
  else QLAUNCH(float, float);
#undef QLAUNCH
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_pca_transform(fhe_ctx* ctx, const float* d_x, int64_t B, int32_t K, const float* d_mean,
                      const float* d_components, int32_t D, float* d_out, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B < 0 || K <= 0 || K > 1024 || D <= 0 || (B > 0 && (!d_x || !d_mean || !d_components || !d_out)))
    return fail(ctx, FHE_E_ARG, "bad pca arguments (1 <= K <= 1024, D >= 1)");
  if (B == 0) return FHE_OK;
  if (B > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, "pca batch too large: split the call");
  hipLaunchKernelGGL(k_pca_transform, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, d_x, (int)K, d_mean,
                     d_components, (int)D, d_out);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_dequantize(fhe_ctx* ctx, const int64_t* d_acc, int64_t B, double out_scale, double* d_score, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B < 0 || (B > 0 && (!d_acc || !d_score))) return fail(ctx, FHE_E_ARG, "bad dequantize arguments");
  if (B == 0) return FHE_OK;
  hipLaunchKernelGGL(k_dequantize, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_acc, B,
                     out_scale, d_score);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_topk(fhe_ctx* ctx, const int64_t* d_acc, const int64_t* d_below, int64_t B, int64_t base_idx, int32_t k,
             int64_t* d_out_acc, int64_t* d_out_idx, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (B < 0 || k < 0 || (k > 0 && (!d_out_acc || !d_out_idx)) || (B > 0 && !d_acc))
    return fail(ctx, FHE_E_ARG, "bad topk arguments");
  if (k == 0) return FHE_OK;
  hipLaunchKernelGGL(k_topk, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_acc, d_below, B, base_idx, k, d_out_acc,
                     d_out_idx);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}

int fhe_dev_alloc(fhe_ctx* ctx, size_t bytes, void** d_out) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!d_out) return fail(ctx, FHE_E_ARG, "null output pointer");
  *d_out = nullptr;
  if (bytes == 0) return FHE_OK;
  if (hipMalloc(d_out, bytes) != hipSuccess) {
    *d_out = nullptr;
    return fail(ctx, FHE_E_NOMEM, "hipMalloc failed");
  }
  return FHE_OK;
}

int fhe_dev_free(fhe_ctx* ctx, void* d_ptr) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (d_ptr) HIPCHK(ctx, hipFree(d_ptr));
  return FHE_OK;
}

int fhe_memcpy_h2d(fhe_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (bytes == 0) return FHE_OK;
  if (!d_dst || !h_src) return fail(ctx, FHE_E_ARG, "null copy pointer");
  HIPCHK(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return FHE_OK;
}

int fhe_memcpy_d2h(fhe_ctx* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (bytes == 0) return FHE_OK;
  if (!h_dst || !d_src) return fail(ctx, FHE_E_ARG, "null copy pointer");
  HIPCHK(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
  return FHE_OK;
}

int fhe_stream_sync(fhe_ctx* ctx, void* stream) {
  int rc = need_device(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
  return FHE_OK;
}

int fhe_debug_v4_stamps(fhe_ctx* ctx, uint64_t* h_out) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!h_out) return fail(ctx, FHE_E_ARG, "null output");
#ifndef FHEICP_AB
  return fail(ctx, FHE_E_STATE, "phase stamps need an A/B build (FHEICP_AB, tools/build_variant.sh)");
#endif
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_v4_stamps), sizeof(unsigned long long) * 64));
  HIPCHK(ctx, hipMemcpyFromSymbol(h_out + 64, HIP_SYMBOL(g_v4_span), sizeof(unsigned long long) * 2048 * 3));
  return FHE_OK;
}

int fhe_debug_el_stamps(fhe_ctx* ctx, uint64_t* h_out) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!h_out) return fail(ctx, FHE_E_ARG, "null output");
#ifndef FHEICP_AB
  return fail(ctx, FHE_E_STATE, "phase stamps need an A/B build (FHEICP_AB, tools/build_variant.sh)");
#else
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_el_stamps), sizeof(unsigned long long) * 1024 * 4 * 10));
  return FHE_OK;
#endif
}

// FHEICP_SRC_SHA: sha256 (first 16 hex digits) of the sources the library was
// compiled from, passed by __graft_entry__.build_lib (tests/test_abi.py checks
// it against the tree, so a stale binary cannot pass for the current one)
#ifndef FHEICP_SRC_SHA
#define FHEICP_SRC_SHA "unknown"
#endif
const char* fhe_build_info(void) {
#ifdef FHEICP_AB
  return "libfheicp gfx950 ab=1 src=" FHEICP_SRC_SHA;
#else
  return "libfheicp gfx950 ab=0 src=" FHEICP_SRC_SHA;
#endif
}

static ProfAcc* prof_bucket(fhe_ctx* ctx, const char* kernel) {
  if (!strcmp(kernel, "blind_rotate") || !strcmp(kernel, "blind_rotate_main")) return &ctx->prof_br;
  if (!strcmp(kernel, "blind_rotate_fast")) return &ctx->prof_brf[0];
  if (!strcmp(kernel, "blind_rotate_fast2")) return &ctx->prof_brf[1];
  if (!strcmp(kernel, "blind_rotate_mid")) return &ctx->prof_brf[2];
  if (!strcmp(kernel, "blind_rotate_mid2")) return &ctx->prof_brf[3];
  if (!strcmp(kernel, "blind_rotate_mid0")) return &ctx->prof_brf[4];
  if (!strcmp(kernel, "keyswitch")) return &ctx->prof_ks;
  if (!strcmp(kernel, "encrypt_linear")) return &ctx->prof_enc;
  if (!strcmp(kernel, "linear_query")) return &ctx->prof_lq;
  if (!strcmp(kernel, "linear_seeded")) return &ctx->prof_ls;
  if (!strcmp(kernel, "pack")) return &ctx->prof_pack;
  if (!strcmp(kernel, "bridge")) return &ctx->prof_bridge;
  if (!strcmp(kernel, "linear_ggsw")) return &ctx->prof_xp;
  if (!strcmp(kernel, "linear_ggsws")) return &ctx->prof_xq;
  if (!strcmp(kernel, "expand_ggsw_seeded")) return &ctx->prof_xs;
  return nullptr;
}

int fhe_profile_kernel_name(fhe_ctx* ctx, const char* kernel, char* h_buf, size_t len) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (!kernel || !h_buf || len == 0) return fail(ctx, FHE_E_ARG, "null kernel name or buffer");
  ProfAcc* a = prof_bucket(ctx, kernel);
  if (!a) return fail(ctx, FHE_E_ARG, "unknown kernel name");
  const char* nm = a->kernel ? a->kernel : "";
  snprintf(h_buf, len, "%s", nm);
  return FHE_OK;
}

int fhe_profile_enable(fhe_ctx* ctx, int enable) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  ctx->prof = enable != 0;
  return FHE_OK;
}

int fhe_profile_read(fhe_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches, int64_t* items) {
  int rc = need_device(ctx);
  if (rc) return rc;
  if (!kernel) return fail(ctx, FHE_E_ARG, "null kernel name");
  std::vector<ProfAcc*> acc;
  if (!strcmp(kernel, "blind_rotate"))
    acc = {&ctx->prof_br, &ctx->prof_brf[0], &ctx->prof_brf[1], &ctx->prof_brf[2], &ctx->prof_brf[3], &ctx->prof_brf[4]};
  else if (ProfAcc* a = prof_bucket(ctx, kernel)) acc = {a};
  else return fail(ctx, FHE_E_ARG, "unknown kernel name");
  double ms = 0;
  int64_t nl = 0, it = 0;
  for (ProfAcc* a : acc) {
    for (auto& e : a->ev) {
      HIPCHK(ctx, hipEventSynchronize(e.second));
      float x = 0;
      HIPCHK(ctx, hipEventElapsedTime(&x, e.first, e.second));
      ms += x;
    }
    nl += a->launches;
    it += a->items;
    free_ev(*a);
    a->launches = 0;
    a->items = 0;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = nl;
  if (items) *items = it;
  return FHE_OK;
}

// ---- several key holders in one batched call -------------
// A group borrows T contexts with equal parameters on one device. Its rows are
// T segments padded to whole four-ciphertext workgroups (fhe_group_rows); per
// round ONE key switch whose workgroups each pick their tenant's key planes
// (k_ks_grp.h, §8.13), then ONE rotation launch whose workgroups each pick
// their tenant's bootstrapping key (k_blind_rotate_*_grp). Timing of the group rotations goes to tenant 0's
// blind-rotation buckets.
struct fhe_group {
  std::vector<fhe_ctx*> ctxs;
  int device = -1;
  const c64** d_keys = nullptr;     // [NGAD + 1][T]: tenant t's bsk_fft of gadget g, then its ksk8 planes
  std::vector<const c64*> h_keys;   // what d_keys holds
  DevBuf ws;                        // tables | small | (search: ct_v | sign | copy | expanded queries / constants)
  DevBuf ks_ws;                     // the group key switch's digit groups | bodies (M words)
  DevBuf bridge_ws;                 // the group bridge's tables | block table | digits | bodies | compact result (§8.18)
  int ks_tiles = 512;               // the key switch's K-split target: two workgroups per CU of the device
};

static int gfail(int code, const std::string& msg) { return fail(nullptr, code, "group: " + msg); }

// the group kernel launch_br's choice for gadget `gad` maps to: 1 multi-bit,
// 2 generic, 0 none (the classic v4 / v4s / two-wave rotations)
static int grp_kernel_for(const fhe_params& cp, int gad) {
  const bool fast = gad > 0 && fast_level(cp, gad);
  const fhe_params p = fast ? fast_params(cp, gad) : cp;
  if (fast && mb_for(cp, gad)) return p.N == 1024 && p.k == 2 && p.pbs_level <= 8 ? 1 : 0;
  if (p.N == 1024) return 0;
  if (((p.N == 256 || p.N == 512) && (p.k == 1 || p.k == 2)) || (p.N == 2048 && p.k == 1)) return 2;
  return 0;
}
static int grp_schedule(const fhe_params& p, int* d, int* sched) {
  *d = 0;
  if (p.msg_bits < 4) {
    for (int r = 0; r < p.msg_bits; ++r) sched[r] = 0;
    return p.msg_bits;
  }
  return sign_schedule(p, d, sched);
}
// the first round of the sign schedule without a group kernel, or -1
static int grp_classic_round(const fhe_params& p) {
  int d, sched[64];
  const int R = grp_schedule(p, &d, sched);
  for (int r = 0; r < R; ++r)
    if (!grp_kernel_for(p, sched[r])) return r;
  return -1;
}
// checks 2 and 3 of fhe_group_create; 2 again at every call (fhe_set_msg_bits)
static int grp_check_params(const fhe_group* g) {
  for (size_t t = 1; t < g->ctxs.size(); ++t)
    if (g->ctxs[t]->device != g->ctxs[0]->device || memcmp(&g->ctxs[t]->p, &g->ctxs[0]->p, sizeof(fhe_params)))
      return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + " differs from tenant 0 in its device or parameters");
  const int r = grp_classic_round(g->ctxs[0]->p);
  if (r >= 0) return gfail(FHE_E_ARG, "round " + std::to_string(r) + " runs the classic rotation (no group kernel)");
  return FHE_OK;
}
static int grp_check_keys(const fhe_group* g) {
  for (size_t t = 0; t < g->ctxs.size(); ++t)
    if (!g->ctxs[t]->keys) return gfail(FHE_E_STATE, "tenant " + std::to_string(t) + " has no evaluation keys");
  if (g->device < 0) return gfail(FHE_E_DEVICE, "host-only contexts");
  if (hipSetDevice(g->device) != hipSuccess) return gfail(FHE_E_DEVICE, "hipSetDevice failed");
  return FHE_OK;
}
// the key-pointer table follows the contexts (a re-keyed tenant moves its keys)
static int grp_sync_keys(fhe_group* g) {
  const size_t T = g->ctxs.size();
  std::vector<const c64*> k((size_t)(NGAD + 1) * T);
  for (int gd = 0; gd < NGAD; ++gd)
    for (size_t t = 0; t < T; ++t) k[gd * T + t] = gd ? g->ctxs[t]->bskf_fft[gd - 1] : g->ctxs[t]->bsk_fft;
  for (size_t t = 0; t < T; ++t) k[(size_t)NGAD * T + t] = (const c64*)g->ctxs[t]->ksk8;  // k_keyswitch_mfma_grp's
  if (k == g->h_keys) return FHE_OK;
  fhe_ctx* c0 = g->ctxs[0];
  HIPCHK(c0, hipDeviceSynchronize());
  if (!g->d_keys) HIPCHK(c0, hipMalloc((void**)&g->d_keys, sizeof(c64*) * k.size()));
  HIPCHK(c0, hipMemcpy(g->d_keys, k.data(), sizeof(c64*) * k.size(), hipMemcpyHostToDevice));
  g->h_keys = k;
  return FHE_OK;
}
static int grp_ensure_ws(fhe_group* g, size_t bytes) {
  return reserve(nullptr, g->ws, bytes, FHE_E_NOMEM, "group: workspace: out of device memory (fewer rows per call)");
}

int64_t fhe_group_rows(const int64_t* counts, int32_t T, int64_t* starts) {
  if (!counts || T < 0) return -1;
  int64_t m = 0;
  for (int32_t t = 0; t < T; ++t) {
    if (counts[t] < 0 || counts[t] > ((int64_t)1 << 40)) return -1;
    if (starts) starts[t] = m;
    m += (counts[t] + 3) / 4 * 4;
  }
  return m;
}

int fhe_group_form(const fhe_params* params) {
  std::string why;
  if (validate(params, why)) return fail(nullptr, FHE_E_ARG, why);
  return grp_classic_round(*params) < 0 ? 1 : 0;
}

int fhe_group_create(fhe_ctx* const* ctxs, int32_t T, fhe_group** out) {
  if (!out) return gfail(FHE_E_ARG, "out is null");
  *out = nullptr;
  if (T < 1 || T > 64 || !ctxs) return gfail(FHE_E_ARG, "1 to 64 contexts");
  for (int32_t t = 0; t < T; ++t) {
    if (!ctxs[t]) return gfail(FHE_E_ARG, "context " + std::to_string(t) + " is null");
    for (int32_t u = 0; u < t; ++u)
      if (ctxs[u] == ctxs[t]) return gfail(FHE_E_ARG, "context " + std::to_string(t) + " repeats context " + std::to_string(u));
  }
  fhe_group* g = new fhe_group();
  g->ctxs.assign(ctxs, ctxs + T);
  g->device = ctxs[0]->device;
  int rc = grp_check_params(g);
  if (!rc) rc = grp_check_keys(g);
  if (!rc) rc = grp_sync_keys(g);
  if (rc) {
    fhe_group_destroy(g);
    return rc;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) == hipSuccess && cus > 0)
    g->ks_tiles = 2 * cus;
  else
    (void)hipGetLastError();
  *out = g;
  return FHE_OK;
}

void fhe_group_destroy(fhe_group* g) {
  if (!g) return;
  if (g->device >= 0 && (g->d_keys || g->ws.p || g->ks_ws.p || g->bridge_ws.p)) {
    (void)hipSetDevice(g->device);
    (void)hipFree((void*)g->d_keys);
    (void)hipFree(g->ws.p);
    (void)hipFree(g->ks_ws.p);
    (void)hipFree(g->bridge_ws.p);
  }
  delete g;
}

// one group rotation over the M padded rows on gadget `gad`
static int launch_br_grp(fhe_group* g, const u64* small, int64_t M, const int32_t* wgt, const BrGrpTenant* ten, BrTv tv,
                         int mode, u64* ct_v, u64* sign, hipStream_t st, int gad) {
  fhe_ctx* c0 = g->ctxs[0];
  const bool fast = gad > 0 && fast_level(c0->p, gad);
  const fhe_params p = fast ? fast_params(c0->p, gad) : c0->p;
  const BrGrpTenant* tg = ten + (size_t)(fast ? gad : 0) * g->ctxs.size();
  ProfAcc& prof = fast ? c0->prof_brf[gad - 1] : c0->prof_br;
  hipEvent_t e1;
  prof_begin(c0, prof, st, &e1);
  const char* name = nullptr;
  if (grp_kernel_for(c0->p, gad) == 1) {
    const dim3 gm((unsigned)(M / 4)), bm(v4::nthreads(4));
#define MBG(L, B)                                                                                                  \
  hipLaunchKernelGGL((k_blind_rotate_mb_grp<L, B>), gm, bm, 0, st, small, wgt, tg, p.n, p.pbs_base_log, c0->tw4,   \
                     c0->psi, tv, mode, ct_v, sign);                                                               \
  name = "k_blind_rotate_mb_grp<" #L ", " #B ">"
#define MB64G(L)                                                                                                   \
  hipLaunchKernelGGL((k_blind_rotate_mb64_grp<L>), gm, bm, 0, st, small, wgt, tg, p.n, p.pbs_base_log, c0->tw4,    \
                     c0->psi, tv, mode, ct_v, sign);                                                               \
  name = "k_blind_rotate_mb64_grp<" #L ">"
    // launch_br's choice among the multi-bit kernels
    if (!(p.pbs_level <= 2 && p.pbs_level * p.pbs_base_log <= 31)) {
      switch (p.pbs_level) {
        case 1: MB64G(1); break;
        case 2: MB64G(2); break;
        case 3: MB64G(3); break;
        case 4: MB64G(4); break;
        case 5: MB64G(5); break;
        case 6: MB64G(6); break;
        case 7: MB64G(7); break;
        default: MB64G(8); break;
      }
    } else if (p.pbs_level == 1 && p.pbs_base_log == 23) {
      MBG(1, 23);
    } else if (p.pbs_level == 1) {
      MBG(1, 0);
    } else if (p.pbs_base_log == 15) {
      MBG(2, 15);
    } else {
      MBG(2, 0);
    }
#undef MBG
#undef MB64G
  } else {
#define BRG(LOGM, K)                                                                                               \
  hipLaunchKernelGGL((k_blind_rotate_grp<LOGM, K>), dim3((unsigned)M), dim3(64), 0, st, small, wgt, tg, p.n,       \
                     p.pbs_level, p.pbs_base_log, c0->tw, c0->twist, tv, mode, ct_v, sign);                        \
  name = "k_blind_rotate_grp<" #LOGM ", " #K ">"
    if (p.N == 256 && p.k == 1) { BRG(7, 1); }
    else if (p.N == 256) { BRG(7, 2); }
    else if (p.N == 512 && p.k == 1) { BRG(8, 1); }
    else if (p.N == 512) { BRG(8, 2); }
    else { BRG(10, 1); }
#undef BRG
  }
  prof.kernel = name;
  prof_end(c0, prof, st, e1, M);
  HIPCHK(c0, hipGetLastError());
  return FHE_OK;
}

// table words before the rows of a group workspace: starts | ends | the
// per-gadget tenant table | the workgroups' tenants (padded to 16 bytes) |
// the key switch's ciphertext blocks (at most M / 128 + T)
static size_t grp_wgt_bytes(int64_t M) { return ((size_t)(M / 4) * 4 + 15) / 16 * 16; }
static size_t grp_table_bytes(size_t T, int64_t M) {
  const size_t blocks = sizeof(KsGrpBlock) * ((size_t)(M / KSM_CTS) + T);  // 24 bytes each
  return 16 * T + sizeof(BrGrpTenant) * NGAD * T + grp_wgt_bytes(M) + (blocks + 15) / 16 * 16;  // rows stay 16-aligned
}
#ifndef FHEICP_GRP_KS
#define FHEICP_GRP_KS 1  // 0: one key switch per tenant, as before the group form (A/B builds)
#endif
// The MFMA key switch of every tenant's rows in two launches (k_ks_grp.h):
// the digits and the GEMM over the ciphertext blocks of `blk`, each with its
// tenant's key planes; keyswitch_lane's split rule on the launch's total of
// blocks x column groups. Timing goes to tenant 0's key-switch bucket.
static int grp_ks_fits(const fhe_group* g, const int64_t* counts);
// the tenants' ciphertext blocks (128 rows) and digit groups (16 rows) together
struct GrpKsCount {
  int64_t nblk = 0, ndg = 0;
};
static GrpKsCount grp_ks_count(const fhe_group* g, const int64_t* counts) {
  GrpKsCount c;
  for (size_t t = 0; t < g->ctxs.size(); ++t) {
    c.nblk += (counts[t] + KSM_CTS - 1) / KSM_CTS;
    c.ndg += (counts[t] + 15) / 16;
  }
  return c;
}
static int grp_keyswitch(fhe_group* g, const u64* d_big, const int64_t* counts, const KsGrpBlock* blk, int64_t M,
                         int32_t shift, uint64_t add_body, u64* d_small, hipStream_t st) {
  fhe_ctx* c0 = g->ctxs[0];
  const fhe_params& p = c0->p;
  const size_t T = g->ctxs.size();
  const auto [nblk, ndg] = grp_ks_count(g, counts);
  if (nblk == 0) return FHE_OK;
  // the digit launch's grid y is 8 per block
  if (ndg > 65535 || 8 * nblk > 65535) return grp_ks_fits(g, counts);  // the entries checked it already
  const int K = p.k * p.N * p.ks_level, KB = K / 64, n1 = p.n + 1, NB = ks_nb(p), CB = ks_cb(p), R = ks_round_bits(p);
  const size_t dbytes = (size_t)ndg * 16 * K, need = dbytes + 8 * (size_t)M;
  int rc = reserve(nullptr, g->ks_ws, need, FHE_E_NOMEM,
                   "group: key-switch workspace: out of device memory (fewer rows per call)");
  if (rc) return rc;
  uint32_t* D = (uint32_t*)g->ks_ws.p;
  u64* body = (u64*)((char*)g->ks_ws.p + dbytes);
  const int64_t ktiles = nblk * (NB / CB);
  const auto [S, kslice] = ksm_split(KB, ktiles, g->ks_tiles);
  const v4i* const* keys = (const v4i* const*)(g->d_keys + (size_t)NGAD * T);
  hipEvent_t e1;
  prof_begin(c0, c0->prof_ks, st, &e1);
  hipLaunchKernelGGL(k_ks_digits_grp, dim3((unsigned)(p.k * p.N / 64), (unsigned)(8 * nblk)), dim3(256), 0, st, d_big,
                     blk, p.k * p.N, p.ks_base_log, p.ks_level, shift, add_body, KB, D, body, S > 1 ? n1 : 0, d_small);
  const dim3 gks((unsigned)(ktiles * S));
  const bool known = ksm_dispatch(8 - R / 8, CB, [&, S = S, kslice = kslice](auto q, auto c) {
    static const std::string name = ksm_name("k_keyswitch_mfma_grp", q, c);  // one per instantiation
    c0->prof_ks.kernel = name.c_str();
    hipLaunchKernelGGL((k_keyswitch_mfma_grp<q, c>), gks, dim3(256), 0, st, (const v4i*)D, keys, blk, body, n1, NB,
                       KB, R, S, kslice, d_small);
  });
  if (!known) return gfail(FHE_E_ARG, "key-switch byte planes out of range");
  int64_t total = 0;
  for (size_t t = 0; t < T; ++t) total += counts[t];
  prof_end(c0, c0->prof_ks, st, e1, total);
  HIPCHK(c0, hipGetLastError());
  return FHE_OK;
}
// the group form serves tenants that all run the MFMA key switch
static bool grp_ks_grouped(const fhe_group* g) {
  if (!FHEICP_GRP_KS) return false;
  for (fhe_ctx* c : g->ctxs)
    if (c->ks_variant != 2) return false;
  return true;
}
// The group key switch's launch limits over all tenants together (the digit
// launch's grid y is 8 per ciphertext block): checked by every group entry
// before any work is queued. The per-tenant loop has keyswitch_lane's own.
static int grp_ks_fits(const fhe_group* g, const int64_t* counts) {
  if (!grp_ks_grouped(g)) return FHE_OK;
  const auto [nblk, ndg] = grp_ks_count(g, counts);
  if (ndg > 65535 || 8 * nblk > 65535)
    return gfail(FHE_E_ARG, "keyswitch batch too large (more than 65535 digit groups of 16 rows, or 8191 blocks of "
                            "128 rows, over all tenants): split the call");
  return FHE_OK;
}
// starts | ends to the front of `tables`, then the key switch's block table
// behind the rotation's tables (stream-ordered)
static int grp_ks_tables(fhe_group* g, const int64_t* counts, const int64_t* starts, int64_t M, void* tables,
                         hipStream_t st, KsGrpBlock** blk) {
  fhe_ctx* c0 = g->ctxs[0];
  const size_t T = g->ctxs.size();
  std::vector<u64> se(2 * T);
  const int64_t nblk = grp_ks_count(g, counts).nblk;
  for (size_t t = 0; t < T; ++t) {
    se[t] = (u64)starts[t];
    se[T + t] = (u64)(starts[t] + counts[t]);
  }
  u64* d_se = (u64*)tables;
  *blk = (KsGrpBlock*)((char*)tables + 16 * T + sizeof(BrGrpTenant) * NGAD * T + grp_wgt_bytes(M));
  int rc = store_words(c0, d_se, se.data(), (int64_t)(2 * T), st);
  if (rc || !nblk) return rc;
  hipLaunchKernelGGL(k_ks_grp_tables, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, (const int64_t*)d_se,
                     (int)T, nblk, *blk);
  HIPCHK(c0, hipGetLastError());
  return FHE_OK;
}
// The sign extraction over the padded rows: sign_extract's rounds, each one
// group key switch (grp_keyswitch; with a tenant on the VALU variant, or in a
// -DFHEICP_GRP_KS=0 build, T key switches on tenant t's rows, key and
// workspace) and one group rotation, on the caller's stream. `tables` holds
// grp_table_bytes.
static int grp_sign(fhe_group* g, u64* ct_v, const int64_t* counts, const int64_t* starts, int64_t M, u64* sign,
                    u64* small, void* tables, hipStream_t st) {
  fhe_ctx* c0 = g->ctxs[0];
  const fhe_params& p = c0->p;
  const size_t T = g->ctxs.size(), Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
  int rc;
  u64* d_se = (u64*)tables;
  BrGrpTenant* ten = (BrGrpTenant*)(d_se + 2 * T);
  int32_t* wgt = (int32_t*)(ten + (size_t)NGAD * T);
  KsGrpBlock* blk;
  if ((rc = grp_ks_tables(g, counts, starts, M, tables, st, &blk))) return rc;
  const bool grouped = grp_ks_grouped(g);
  const int64_t nwg = M / 4, nth = std::max<int64_t>(nwg, (int64_t)(NGAD * T));
  hipLaunchKernelGGL(k_grp_tables, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, st, g->d_keys,
                     (const int64_t*)d_se, (int)T, NGAD, nwg, ten, wgt);
  HIPCHK(c0, hipGetLastError());
  int d, sched[64], round = 0;
  grp_schedule(p, &d, sched);
  auto step = [&](int shift, uint64_t add, BrTv tv, int mode, uint64_t* sg) -> int {
    if (grouped) {
      int r = grp_keyswitch(g, ct_v, counts, blk, M, shift, add, small, st);
      if (r) return r;
    }
    for (size_t t = 0; t < T && !grouped; ++t) {
      if (!counts[t]) continue;
      int r = keyswitch_lane(g->ctxs[t], ct_v + (size_t)starts[t] * Wb, counts[t], shift, add,
                             small + (size_t)starts[t] * Ws, st, 0);
      if (r) return r;
    }
    return launch_br_grp(g, small, M, wgt, ten, tv, mode, ct_v, sg, st, sched[round++]);
  };
  return sign_walk(p, d, step, sign);
}

// what every group call checks first: counts, then parameters, keys, tables
static int grp_enter(fhe_group* g) {
  int rc = grp_check_params(g);
  if (!rc) rc = grp_check_keys(g);
  if (!rc) rc = grp_sync_keys(g);
  return rc;
}

int fhe_sign_group_batch(fhe_group* g, uint64_t* d_ct_v, const int64_t* h_counts, uint64_t* d_sign, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  const int32_t T = (int32_t)g->ctxs.size();
  std::vector<int64_t> starts((size_t)T);
  const int64_t M = fhe_group_rows(h_counts, T, starts.data());  // < 0: null or a count outside [0, 2^40]
  int64_t total = 0;
  for (int32_t t = 0; M >= 0 && t < T; ++t) total += h_counts[t];
  if (M < 0 || total >= ((int64_t)1 << 31))
    return gfail(FHE_E_ARG, "bad sign arguments (counts null, negative or 2^31 rows and more)");
  int rc = grp_enter(g);
  if (rc) return rc;
  if (M == 0) return FHE_OK;
  if (!d_ct_v || !d_sign) return gfail(FHE_E_ARG, "null sign buffers");
  if ((rc = grp_ks_fits(g, h_counts))) return rc;
  const size_t tb = grp_table_bytes((size_t)T, M);
  if ((rc = grp_ensure_ws(g, tb + 8 * (size_t)M * fhe_small_lwe_words(&g->ctxs[0]->p)))) return rc;
  return grp_sign(g, d_ct_v, h_counts, starts.data(), M, d_sign, (u64*)((char*)g->ws.p + tb), g->ws.p, (hipStream_t)stream);
}

int fhe_keyswitch_group_batch(fhe_group* g, const uint64_t* d_big, const int64_t* h_counts, int32_t shift,
                              uint64_t add_body, uint64_t* d_small, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  const int32_t T = (int32_t)g->ctxs.size();
  std::vector<int64_t> starts((size_t)T);
  const int64_t M = fhe_group_rows(h_counts, T, starts.data());  // < 0: null or a count outside [0, 2^40]
  int64_t total = 0;
  for (int32_t t = 0; M >= 0 && t < T; ++t) total += h_counts[t];
  if (M < 0 || total >= ((int64_t)1 << 31))
    return gfail(FHE_E_ARG, "bad keyswitch arguments (counts null, negative or 2^31 rows and more)");
  if (shift < 0 || shift > ks_max_shift(g->ctxs[0]->p))
    return gfail(FHE_E_ARG, "bad keyswitch arguments (shift must be in [0, 63 - ks_level * (ks_base_log + 1)])");
  int rc = grp_enter(g);
  if (rc) return rc;
  if (M == 0) return FHE_OK;
  if (!d_big || !d_small) return gfail(FHE_E_ARG, "null keyswitch buffers");
  if ((rc = grp_ks_fits(g, h_counts))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const fhe_params& p = g->ctxs[0]->p;
  if (!grp_ks_grouped(g)) {
    const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p);
    for (int32_t t = 0; t < T; ++t) {
      if (!h_counts[t]) continue;
      if ((rc = keyswitch_lane(g->ctxs[t], d_big + (size_t)starts[t] * Wb, h_counts[t], shift, add_body,
                               d_small + (size_t)starts[t] * Ws, st, 0)))
        return rc;
    }
    return FHE_OK;
  }
  if ((rc = grp_ensure_ws(g, grp_table_bytes((size_t)T, M)))) return rc;
  KsGrpBlock* blk;
  if ((rc = grp_ks_tables(g, h_counts, starts.data(), M, g->ws.p, st, &blk))) return rc;
  return grp_keyswitch(g, d_big, h_counts, blk, M, shift, add_body, d_small, st);
}

int fhe_search_query_group_batch(fhe_group* g, const fhe_group_query* items, int32_t T, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  if (!items || T != (int32_t)g->ctxs.size()) return gfail(FHE_E_ARG, "one fhe_group_query per tenant");
  // argument errors first, before any device or key is looked at
  std::vector<int64_t> counts((size_t)T), starts((size_t)T);
  int64_t total = 0;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_query& q = items[t];
    if (q.struct_size != (int32_t)sizeof(fhe_group_query))
      return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": fhe_group_query.struct_size is not this library's");
    if (q.Q < 0) return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": Q < 0");
    counts[t] = 0;
    if (q.Q == 0) continue;  // sits this call out
    if (queries_args(g->ctxs[t], q.Q, q.B, q.D)) return FHE_E_ARG;
    if (q.levels_bit < 0 || q.levels_bit > 8)
      return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": levels_bit outside [0, 8]");
    counts[t] = q.Q * q.B;
    total += counts[t];
    if (total >= ((int64_t)1 << 31)) return gfail(FHE_E_ARG, "2^31 results and more: split the call");
  }
  int rc = grp_enter(g);
  if (rc) return rc;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_query& q = items[t];
    if (!q.Q) continue;
    if ((rc = need_pack_key(g->ctxs[t]))) return rc;
    if (q.levels_bit > g->ctxs[t]->pack_key.level)
      return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": levels_bit exceeds the packing key's levels");
    if (!q.h_mask_key || !q.h_T || !q.d_qbody || !q.d_id0 || !q.d_docs8 || !q.d_w || !q.d_glwe_acc || !q.d_glwe_bit)
      return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": null search arguments");
  }
  const int64_t M = fhe_group_rows(counts.data(), T, starts.data());
  if (M == 0) return FHE_OK;
  if ((rc = grp_ks_fits(g, counts.data()))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const fhe_params& p = g->ctxs[0]->p;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p), tb = grp_table_bytes((size_t)T, M);
  size_t qmax = 0;  // the largest tenant's expanded queries (one at a time, in stream order)
  for (int32_t t = 0; t < T; ++t) qmax = std::max(qmax, (size_t)items[t].Q * (size_t)items[t].D * Wb);
  if ((rc = grp_ensure_ws(g, tb + 8 * ((size_t)M * (3 * Wb + Ws) + qmax)))) return rc;
  u64* small = (u64*)((char*)g->ws.p + tb);
  u64* ctv = small + (size_t)M * Ws;
  u64* sgn = ctv + (size_t)M * Wb;
  u64* cpy = sgn + (size_t)M * Wb;
  u64* ctq = cpy + (size_t)M * Wb;
  // per tenant: expansion and leveled GEMM into its segment, a copy of the
  // leveled rows (the sign extraction consumes them)
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_query& q = items[t];
    if (!q.Q) continue;
    fhe_ctx* ctx = g->ctxs[t];
    std::vector<int64_t> cs((size_t)q.Q);
    for (int64_t i = 0; i < q.Q; ++i) cs[(size_t)i] = q.cst - q.h_T[i];
    if ((rc = fhe_expand_seeded_batch(ctx, q.d_qbody, q.d_id0, q.Q, q.D, q.h_mask_key, ctq, stream))) return rc;
    u64* seg = ctv + (size_t)starts[t] * Wb;
    if ((rc = fhe_linear_queries_batch(ctx, ctq, q.Q, q.d_docs8, q.B, q.D, q.d_w, cs.data(), seg, stream))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(cpy + (size_t)starts[t] * Wb, seg, 8 * (size_t)counts[t] * Wb, hipMemcpyDeviceToDevice, st));
  }
  if ((rc = grp_sign(g, ctv, counts.data(), starts.data(), M, sgn, small, g->ws.p, st))) return rc;
  // tenant t's two packings with its own key: result q B + b in coefficient
  // (q B + b) mod N of its GLWE (q B + b) / N, as fhe_search_queries_batch
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_query& q = items[t];
    if (!q.Q) continue;
    fhe_ctx* ctx = g->ctxs[t];
    if ((rc = pack_impl(ctx, cpy + (size_t)starts[t] * Wb, counts[t], ctx->pack_key.level, q.d_glwe_acc, st))) return rc;
    if ((rc = pack_impl(ctx, sgn + (size_t)starts[t] * Wb, counts[t], q.levels_bit ? q.levels_bit : ctx->pack_key.level,
                        q.d_glwe_bit, st)))
      return rc;
  }
  return FHE_OK;
}

// ---- stored-ciphertext search for a group ----------------
int fhe_search_seeded_queries_group_batch(fhe_group* g, const fhe_group_corpus* items, int32_t T, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  if (!items || T != (int32_t)g->ctxs.size()) return gfail(FHE_E_ARG, "one fhe_group_corpus per tenant");
  // argument errors first, before any device or key is looked at
  std::vector<int64_t> counts((size_t)T), starts((size_t)T);
  int64_t total = 0, qmax = 0;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus& c = items[t];
    const std::string who = "tenant " + std::to_string(t) + ": ";
    if (c.struct_size != (int32_t)sizeof(fhe_group_corpus))
      return gfail(FHE_E_ARG, who + "fhe_group_corpus.struct_size is not this library's");
    if (c.Q < 0) return gfail(FHE_E_ARG, who + "Q < 0");
    counts[t] = 0;
    if (c.Q == 0) continue;  // sits this call out
    if (seeded_queries_args(g->ctxs[t], c.Q, c.B, c.D))
      return gfail(FHE_E_ARG, who + fhe_last_error(g->ctxs[t]));
    if (c.levels_bit < 0 || c.levels_bit > 8) return gfail(FHE_E_ARG, who + "levels_bit outside [0, 8]");
    if (!c.d_body || !c.d_id0 || !c.h_mask_key || !c.d_W || !c.h_T || !c.d_glwe_acc || !c.d_glwe_bit)
      return gfail(FHE_E_ARG, who + "null search arguments");
    if (c.B_old < 0 || c.B_old > c.B) return gfail(FHE_E_ARG, who + "B_old outside [0, B]");
    counts[t] = c.Q * c.B;
    total += counts[t];
    qmax = std::max(qmax, c.Q);
    if (total >= ((int64_t)1 << 31)) return gfail(FHE_E_ARG, "2^31 results and more: split the call");
  }
  int rc = grp_enter(g);
  if (rc) return rc;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus& c = items[t];
    if (!c.Q) continue;
    const std::string who = "tenant " + std::to_string(t) + ": ";
    if ((rc = need_pack_key(g->ctxs[t]))) return gfail(rc, who + fhe_last_error(g->ctxs[t]));
    if (c.B_old > 0 && (rc = need_bridge_key(g->ctxs[t]))) return gfail(rc, who + fhe_last_error(g->ctxs[t]));
    if (c.levels_bit > g->ctxs[t]->pack_key.level)
      return gfail(FHE_E_ARG, who + "levels_bit exceeds the packing key's levels");
  }
  const int64_t M = fhe_group_rows(counts.data(), T, starts.data());
  if (M == 0) return FHE_OK;
  if ((rc = grp_ks_fits(g, counts.data()))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const fhe_params& p = g->ctxs[0]->p;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p), tb = grp_table_bytes((size_t)T, M);
  if ((rc = grp_ensure_ws(g, tb + 8 * ((size_t)M * (3 * Wb + Ws) + (size_t)qmax)))) return rc;
  u64* small = (u64*)((char*)g->ws.p + tb);
  u64* ctv = small + (size_t)M * Ws;
  u64* sgn = ctv + (size_t)M * Wb;
  u64* cpy = sgn + (size_t)M * Wb;
  u64* dcs = cpy + (size_t)M * Wb;  // one tenant's scaled constants at a time, in stream order
  // per tenant: the leveled step into its segment, the bridge on its old
  // documents' rows, a copy of the leveled rows (the sign extraction consumes them)
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus& c = items[t];
    if (!c.Q) continue;
    fhe_ctx* ctx = g->ctxs[t];
    u64* seg = ctv + (size_t)starts[t] * Wb;
    if ((rc = store_scaled_csts(ctx, dcs, c.Q, nullptr, c.cst, c.h_T, st))) return rc;
    if ((rc = linear_seeded_queries_launch(ctx, c.d_body, c.d_id0, c.B, c.D, c.h_mask_key, c.Q, c.d_W, dcs, seg, st)))
      return rc;
    if (c.B_old > 0 && (rc = bridge_impl(ctx, ctx->bridge_keys[0], seg, c.Q, c.B, c.B_old, seg, st))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(cpy + (size_t)starts[t] * Wb, seg, 8 * (size_t)counts[t] * Wb, hipMemcpyDeviceToDevice, st));
  }
  if ((rc = grp_sign(g, ctv, counts.data(), starts.data(), M, sgn, small, g->ws.p, st))) return rc;
  // tenant t's two packings with its own key, as fhe_search_seeded_queries_bridged_batch
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus& c = items[t];
    if (!c.Q) continue;
    fhe_ctx* ctx = g->ctxs[t];
    if ((rc = pack_impl(ctx, cpy + (size_t)starts[t] * Wb, counts[t], ctx->pack_key.level, c.d_glwe_acc, st))) return rc;
    if ((rc = pack_impl(ctx, sgn + (size_t)starts[t] * Wb, counts[t], c.levels_bit ? c.levels_bit : ctx->pack_key.level,
                        c.d_glwe_bit, st)))
      return rc;
  }
  return FHE_OK;
}

// ---- rotation schedules in a group: one bridge for all tenants (§8.18) -----
// One tenant's row map as the two entries below hand it over.
struct GrpRowMap {
  int64_t Q = 0, B = 0;  // Q = 0: the tenant sits this call out
  int32_t G = 0;
  const int64_t* h_ends = nullptr;
  const int32_t* h_slots = nullptr;
};
// After the device and key checks and before anything is queued: every named
// slot with rows holds a key (FHE_E_STATE naming tenant and slot), a tenant's
// keys share one gadget (FHE_E_STATE), then the launch limits of every pass
// (FHE_E_ARG). Fills the passes, one per distinct gadget in order of first
// appearance; starts: fhe_group_rows' for counts[t] = Q_t B_t.
static int grp_bridge_plan(const fhe_group* g, const std::vector<GrpRowMap>& maps, const int64_t* starts,
                           std::vector<BridgePass>* passes) {
  passes->clear();
  for (size_t t = 0; t < maps.size(); ++t) {
    const GrpRowMap& m = maps[t];
    if (!m.Q) continue;
    int rc = for_gen_keys(
        g->ctxs[t], m.G, m.h_ends, m.h_slots, true,
        [&](int code, const std::string& msg) { return gfail(code, "tenant " + std::to_string(t) + ": " + msg); },
        [&](int, const GadgetKey& k, int64_t d0, int64_t n) {
          BridgePass* ps = nullptr;
          for (BridgePass& q : *passes)
            if (q.beta == k.beta && q.level == k.level) ps = &q;
          if (!ps) {
            passes->emplace_back();
            ps = &passes->back();
            ps->beta = k.beta;
            ps->level = k.level;
          }
          ps->add(m.Q, n, d0, m.B, starts[t], k.planes);
          return (int)FHE_OK;
        });
    if (rc) return rc;
  }
  for (const BridgePass& ps : *passes)
    if (!ps.fits())
      return gfail(FHE_E_ARG, "bridge batch too large (more than 65535 digit groups of 16 rows, or 8191 blocks of "
                              "128 rows, over all segments of a pass): split the call");
  return FHE_OK;
}
// The passes of a plan on the group's padded rows d_ct, in place, one after
// the other in the group's bridge workspace (the largest pass's). Timing goes
// to the "bridge" bucket of the group's first context, one bracket per pass.
static int grp_bridge_launch(fhe_group* g, u64* d_ct, const std::vector<BridgePass>& passes, hipStream_t st) {
  fhe_ctx* c0 = g->ctxs[0];
  const int big = c0->p.k * c0->p.N;
  size_t need = 0, off[5];
  for (const BridgePass& ps : passes) {
    ps.layout(big, off);
    need = std::max(need, off[4]);
  }
  int rc = reserve(nullptr, g->bridge_ws, need, FHE_E_NOMEM,
                   "group: bridge workspace: out of device memory (fewer rows per call)");
  if (rc) return rc;
  for (const BridgePass& ps : passes)
    if ((rc = bridge_pass_launch(c0, (char*)g->bridge_ws.p, d_ct, ps, st))) return rc;
  return FHE_OK;
}
// the row-map rules of one participating tenant (FHE_E_ARG, "tenant t: ...")
static int grp_rowmap_args(const fhe_group* g, int32_t t, const GrpRowMap& m) {
  fhe_ctx* ctx = g->ctxs[t];
  if (gens_args(ctx, m.B, m.G, m.h_ends, m.h_slots))
    return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": " + fhe_last_error(ctx));
  return FHE_OK;
}

int fhe_bridge_group_gens_batch(fhe_group* g, uint64_t* d_ct, const fhe_group_rowmap* maps, int32_t T, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  if (!maps || T != (int32_t)g->ctxs.size()) return gfail(FHE_E_ARG, "one fhe_group_rowmap per tenant");
  // argument errors first, before any device or key is looked at
  std::vector<int64_t> counts((size_t)T), starts((size_t)T);
  std::vector<GrpRowMap> rm((size_t)T);
  int64_t total = 0;
  int rc;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_rowmap& m = maps[t];
    const std::string who = "tenant " + std::to_string(t) + ": ";
    if (m.struct_size != (int32_t)sizeof(fhe_group_rowmap))
      return gfail(FHE_E_ARG, who + "fhe_group_rowmap.struct_size is not this library's");
    if (m.Q < 0) return gfail(FHE_E_ARG, who + "Q < 0");
    counts[t] = 0;
    if (m.Q == 0) continue;  // sits this call out
    if (m.B < 1 || m.Q > 0x7fffffffLL || m.B > 0x7fffffffLL || m.Q * m.B > 0x7fffffffLL)
      return gfail(FHE_E_ARG, who + "bad bridge generations arguments (Q < 1, B < 1 or Q*B >= 2^31)");
    rm[t].Q = m.Q, rm[t].B = m.B, rm[t].G = m.G, rm[t].h_ends = m.h_ends, rm[t].h_slots = m.h_slots;
    if ((rc = grp_rowmap_args(g, t, rm[t]))) return rc;
    if (!d_ct) return gfail(FHE_E_ARG, who + "null bridge buffers");
    counts[t] = m.Q * m.B;
    total += counts[t];
    if (total >= ((int64_t)1 << 31)) return gfail(FHE_E_ARG, "2^31 results and more: split the call");
  }
  if ((rc = grp_enter(g))) return rc;
  fhe_group_rows(counts.data(), T, starts.data());
  std::vector<BridgePass> passes;
  if ((rc = grp_bridge_plan(g, rm, starts.data(), &passes))) return rc;
  return grp_bridge_launch(g, d_ct, passes, (hipStream_t)stream);
}

// fhe_search_seeded_queries_group_batch with every tenant's generation row map
// in B_old's place: the leveled steps, ONE grouped bridge over all tenants'
// old generations, the copies, one sign extraction, the packings.
int fhe_search_seeded_queries_group_gens_batch(fhe_group* g, const fhe_group_corpus_gens* items, int32_t T,
                                               void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  if (!items || T != (int32_t)g->ctxs.size()) return gfail(FHE_E_ARG, "one fhe_group_corpus_gens per tenant");
  // argument errors first, before any device or key is looked at
  std::vector<int64_t> counts((size_t)T), starts((size_t)T);
  std::vector<GrpRowMap> rm((size_t)T);
  int64_t total = 0, qmax = 0;
  int rc;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus_gens& c = items[t];
    const std::string who = "tenant " + std::to_string(t) + ": ";
    if (c.struct_size != (int32_t)sizeof(fhe_group_corpus_gens))
      return gfail(FHE_E_ARG, who + "fhe_group_corpus_gens.struct_size is not this library's");
    if (c.Q < 0) return gfail(FHE_E_ARG, who + "Q < 0");
    counts[t] = 0;
    if (c.Q == 0) continue;  // sits this call out
    if (seeded_queries_args(g->ctxs[t], c.Q, c.B, c.D))
      return gfail(FHE_E_ARG, who + fhe_last_error(g->ctxs[t]));
    if (c.levels_bit < 0 || c.levels_bit > 8) return gfail(FHE_E_ARG, who + "levels_bit outside [0, 8]");
    rm[t].Q = c.Q, rm[t].B = c.B, rm[t].G = c.G, rm[t].h_ends = c.h_ends, rm[t].h_slots = c.h_slots;
    if ((rc = grp_rowmap_args(g, t, rm[t]))) return rc;
    if (!c.d_body || !c.d_id0 || !c.h_mask_key || !c.d_W || !c.h_T || !c.d_glwe_acc || !c.d_glwe_bit)
      return gfail(FHE_E_ARG, who + "null search arguments");
    counts[t] = c.Q * c.B;
    total += counts[t];
    qmax = std::max(qmax, c.Q);
    if (total >= ((int64_t)1 << 31)) return gfail(FHE_E_ARG, "2^31 results and more: split the call");
  }
  if ((rc = grp_enter(g))) return rc;
  for (int32_t t = 0; t < T; ++t) {
    if (!items[t].Q) continue;
    if ((rc = need_pack_key(g->ctxs[t])))
      return gfail(rc, "tenant " + std::to_string(t) + ": " + fhe_last_error(g->ctxs[t]));
  }
  const int64_t M = fhe_group_rows(counts.data(), T, starts.data());
  std::vector<BridgePass> passes;
  if ((rc = grp_bridge_plan(g, rm, starts.data(), &passes))) return rc;
  for (int32_t t = 0; t < T; ++t)
    if (items[t].Q && items[t].levels_bit > g->ctxs[t]->pack_key.level)
      return gfail(FHE_E_ARG, "tenant " + std::to_string(t) + ": levels_bit exceeds the packing key's levels");
  if (M == 0) return FHE_OK;
  if ((rc = grp_ks_fits(g, counts.data()))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const fhe_params& p = g->ctxs[0]->p;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p), tb = grp_table_bytes((size_t)T, M);
  if ((rc = grp_ensure_ws(g, tb + 8 * ((size_t)M * (3 * Wb + Ws) + (size_t)qmax)))) return rc;
  u64* small = (u64*)((char*)g->ws.p + tb);
  u64* ctv = small + (size_t)M * Ws;
  u64* sgn = ctv + (size_t)M * Wb;
  u64* cpy = sgn + (size_t)M * Wb;
  u64* dcs = cpy + (size_t)M * Wb;  // one tenant's scaled constants at a time, in stream order
  // per tenant the leveled step into its segment; the grouped bridge on every
  // tenant's old documents' rows; then the copies of the leveled rows (the
  // sign extraction consumes them)
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus_gens& c = items[t];
    if (!c.Q) continue;
    fhe_ctx* ctx = g->ctxs[t];
    if ((rc = store_scaled_csts(ctx, dcs, c.Q, nullptr, c.cst, c.h_T, st))) return rc;
    if ((rc = linear_seeded_queries_launch(ctx, c.d_body, c.d_id0, c.B, c.D, c.h_mask_key, c.Q, c.d_W, dcs,
                                           ctv + (size_t)starts[t] * Wb, st)))
      return rc;
  }
  if ((rc = grp_bridge_launch(g, ctv, passes, st))) return rc;
  for (int32_t t = 0; t < T; ++t) {
    if (!items[t].Q) continue;
    HIPCHK(g->ctxs[t], hipMemcpyAsync(cpy + (size_t)starts[t] * Wb, ctv + (size_t)starts[t] * Wb,
                                      8 * (size_t)counts[t] * Wb, hipMemcpyDeviceToDevice, st));
  }
  if ((rc = grp_sign(g, ctv, counts.data(), starts.data(), M, sgn, small, g->ws.p, st))) return rc;
  // tenant t's two packings with its own key, as fhe_search_seeded_queries_gens_batch
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_corpus_gens& c = items[t];
    if (!c.Q) continue;
    fhe_ctx* ctx = g->ctxs[t];
    if ((rc = pack_impl(ctx, cpy + (size_t)starts[t] * Wb, counts[t], ctx->pack_key.level, c.d_glwe_acc, st))) return rc;
    if ((rc = pack_impl(ctx, sgn + (size_t)starts[t] * Wb, counts[t], c.levels_bit ? c.levels_bit : ctx->pack_key.level,
                        c.d_glwe_bit, st)))
      return rc;
  }
  return FHE_OK;
}

// ---- the segmented transposed external product (k_extprod_grp.h) ----------
// What one call's leveled step launches over its segments (the participating
// tenants of a group, §8.14; the generations with documents of a context,
// §8.19): the records, the launch's RT, tile and row-tile counts, the K split
// and the layout of its workspace (tables | constants | planes | results, each
// 16-aligned). RT and L are set before the first add().
struct XqWs {
  XqGrpTenant* ten;
  XqGrpTile* tiles;
  int32_t *rtt, *qdt;  // row tile -> segment, row quad -> segment
  int64_t* ends;
  u64* cst;
  v4i* P8;
  u64* M;
};
struct XqPlan {
  int ns = 0, RT = 1, L = 0, KB = 0, Sk = 1, kslice = 0;
  int64_t ntiles = 0, nrt = 0, mwords = 0, nquads = 0;
  bool with_ends = false;
  XqSegs<XQ_GRP_MAX> seg;
  size_t off_tiles = 0, off_rt = 0, off_quad = 0, off_ends = 0, off_cst = 0, off_planes = 0, off_M = 0, bytes = 0;
  // Q queries (GGSWs at d_ggsw, their constants from c0 on) against the B packed documents at
  // d_docs, D features each; `start`: where the form's extraction puts the segment
  void add(const fhe_params& p, const uint64_t* d_ggsw, const void* d_docs, int64_t start, int64_t Q, int64_t B,
           int32_t D, int64_t c0) {
    const int64_t G = ggsw_glwes(p, B, D), rtp = xq_grp_rtiles(p.k, (int)Q, RT);
    seg.v[ns++] = {d_ggsw, (const uint8_t*)d_docs, start, mwords, (int32_t)Q, (int32_t)G, (int32_t)B, D, (int32_t)nrt,
                   (int32_t)c0};
    ntiles += xq_grp_cgrid(p.N, (int)G) * (rtp / RT);
    nrt += rtp;
    mwords += Q * G * (p.k + 1) * p.N;
  }
  // The split and the layout, for `quads` row quads of a padded output (0: none), an ends table
  // or none, and ncst constants. False when the launch has 2^31 tiles or (row tile, k-block)
  // pairs and more: the tiles are the GEMM's grid x, the pairs the planes'.
  bool finish(const fhe_params& p, int64_t quads, bool ends, int64_t ncst) {
    const int n1 = (p.k + 1) * p.N;
    KB = n1 * L / 64;
    if (ntiles > 0x7fffffffLL || nrt * KB > 0x7fffffffLL) return false;
    const auto [S, ks] = xq_ksplit(KB, ntiles);
    Sk = S, kslice = ks, nquads = quads, with_ends = ends;
    off_tiles = up16(sizeof(XqGrpTenant) * (size_t)ns);
    off_rt = off_tiles + sizeof(XqGrpTile) * (size_t)ntiles;
    off_quad = off_rt + up16(4 * (size_t)nrt);
    off_ends = off_quad + up16(4 * (size_t)nquads);
    off_cst = off_ends + (ends ? up16(8 * (size_t)ns) : 0);
    // the planes' 1 KB fragment runs and the results' 128-byte store runs on whole cache lines
    off_planes = (off_cst + 8 * (size_t)ncst + 255) / 256 * 256;
    off_M = off_planes + (size_t)nrt * 16 * n1 * L * 8;
    bytes = off_M + 8 * (size_t)mwords;
    return true;
  }
  XqWs at(void* ws) const {
    char* w = (char*)ws;
    return {(XqGrpTenant*)w,         (XqGrpTile*)(w + off_tiles),
            (int32_t*)(w + off_rt),  nquads ? (int32_t*)(w + off_quad) : nullptr,
            with_ends ? (int64_t*)(w + off_ends) : nullptr,
            (u64*)(w + off_cst),     (v4i*)(w + off_planes),
            (u64*)(w + off_M)};
  }
};
// The leveled step of every segment in the pl.bytes at `ws` the caller
// reserved, its constants already queued to at(ws).cst: in one bracket of
// ctx's "linear_ggsws" bucket (items = the call's results) the tables, the
// memset of a split K, the planes, the GEMM and the form's extraction,
// extract(at(ws)). The launch count does not depend on the segments.
extern "C++" {
template <class Extract>
static int xq_launch(fhe_ctx* ctx, const XqPlan& pl, void* ws, int64_t items, Extract&& extract, hipStream_t st) {
  const fhe_params& p = ctx->p;
  const XqWs w = pl.at(ws);
  hipEvent_t e1;
  prof_begin(ctx, ctx->prof_xq, st, &e1);
  ctx->prof_xq.kernel = pl.RT == 2 ? "k_extprod_queries_mfma_grp<2>" : "k_extprod_queries_mfma_grp<1>";
  const int64_t nth = std::max(std::max(pl.ntiles, pl.nrt), std::max<int64_t>(pl.nquads, pl.ns));
  auto tables = [&](const auto& segs) {
    hipLaunchKernelGGL(k_xq_tables, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, st, segs, pl.ns, p.N, p.k,
                       pl.RT, pl.ntiles, pl.nrt, pl.nquads, w.ten, w.tiles, w.rtt, w.qdt, w.ends);
  };
  if (pl.ns <= XQ_GENS_MAX) {  // the short argument: every generations call, and a group call of few tenants
    XqSegs<XQ_GENS_MAX> few;
    std::copy(pl.seg.v, pl.seg.v + XQ_GENS_MAX, few.v);
    tables(few);
  } else {
    tables(pl.seg);
  }
  if (pl.Sk > 1) HIPCHK(ctx, hipMemsetAsync(w.M, 0, 8 * (size_t)pl.mwords, st));
  hipLaunchKernelGGL(k_ggsws_planes_grp, dim3((unsigned)(pl.nrt * pl.KB)), dim3(64), 0, st,
                     (const XqGrpTenant*)w.ten, (const int32_t*)w.rtt, p.N, p.k, pl.L, pl.KB, w.P8);
  xq_dispatch(pl.RT, [&](auto rt) {
    hipLaunchKernelGGL(k_extprod_queries_mfma_grp<decltype(rt)::value>, dim3((unsigned)pl.ntiles, 1, (unsigned)pl.Sk),
                       dim3(256), 0, st, (const XqGrpTile*)w.tiles, (const XqGrpTenant*)w.ten, (const v4i*)w.P8, p.N,
                       p.k, pl.L, pl.KB, pl.kslice, w.M);
  });
  extract(w);
  prof_end(ctx, ctx->prof_xq, st, e1, items);
  HIPCHK(ctx, hipGetLastError());
  return FHE_OK;
}
}  // extern "C++"

// ---- both-private search for a group ---------------------
// The group's part of a call's plan: the segments are the participating
// tenants (record -> tenant), with their result counts and their starts in
// the padded layout of M rows.
struct XqGrpPlan {
  XqPlan x;
  int64_t M = 0, total = 0;
  int32_t tenant[XQ_GRP_MAX];  // record -> tenant of the group
  std::vector<int64_t> counts, starts;
};
// The argument checks of both entries (FHE_E_ARG, "tenant t: ...", host-only
// contexts report them too) and the plan. `search`: the thresholds, levels_bit
// and the two outputs are arguments too.
static int xq_grp_plan(fhe_group* g, const fhe_group_ggsw* items, int32_t T, const int64_t* const* h_cst, bool search,
                       XqGrpPlan* pl) {
  pl->counts.assign((size_t)T, 0);
  pl->starts.assign((size_t)T, 0);
  int nt = 0;
  for (int32_t t = 0; t < T; ++t) {
    const fhe_group_ggsw& it = items[t];
    fhe_ctx* ctx = g->ctxs[t];
    const std::string who = "tenant " + std::to_string(t) + ": ";
    if (it.struct_size != (int32_t)sizeof(fhe_group_ggsw))
      return gfail(FHE_E_ARG, who + "fhe_group_ggsw.struct_size is not this library's");
    if (it.Q < 0) return gfail(FHE_E_ARG, who + "Q < 0");
    if (it.Q == 0) continue;  // sits this call out
    if (it.reserved != 0) return gfail(FHE_E_ARG, who + "fhe_group_ggsw.reserved is not 0");
    if (ggsws_args(ctx, it.Q, it.B, it.D, it.base_log, it.level)) return gfail(FHE_E_ARG, who + fhe_last_error(ctx));
    if (!it.d_ggsw || !it.d_docs) return gfail(FHE_E_ARG, who + "null ggsw queries or documents");
    if (search) {
      if (!it.h_T || !it.d_glwe_acc || !it.d_glwe_bit) return gfail(FHE_E_ARG, who + "null search arguments");
      if (it.levels_bit < 0 || it.levels_bit > 8) return gfail(FHE_E_ARG, who + "levels_bit outside [0, 8]");
    } else if (!h_cst[t]) {
      return gfail(FHE_E_ARG, who + "null constants");
    }
    if (nt && it.level != pl->x.L)
      return gfail(FHE_E_ARG, who + "gadget level " + std::to_string(it.level) + " differs from the first participating "
                                  "tenant's " + std::to_string(pl->x.L) + ": one level per call");
    pl->x.L = it.level;
    pl->counts[t] = it.Q * it.B;
    pl->total += pl->counts[t];
    if (pl->total >= ((int64_t)1 << 31)) return gfail(FHE_E_ARG, "2^31 results and more: split the call");
    pl->tenant[nt++] = t;
  }
  pl->M = fhe_group_rows(pl->counts.data(), T, pl->starts.data());
  if (!nt) return FHE_OK;
  const fhe_params& p = g->ctxs[0]->p;  // the contexts' parameters are equal (grp_check_params, before any launch)
  for (int i = 0; i < nt; ++i)
    if (items[pl->tenant[i]].Q * (p.k + 1) > 16) pl->x.RT = 2;
  int64_t nq = 0;
  for (int i = 0; i < nt; ++i) {
    const int32_t t = pl->tenant[i];
    const fhe_group_ggsw& it = items[t];
    pl->x.add(p, it.d_ggsw, it.d_docs, pl->starts[t], it.Q, it.B, it.D, nq);
    nq += it.Q;
  }
  if (!pl->x.finish(p, pl->M / 4, false, nq))
    return gfail(FHE_E_ARG, "ggsw queries batch too large (2^31 tiles over all tenants): split the call");
  return FHE_OK;
}
// The leveled step of every participating tenant at `ws` (pl.x.bytes of the
// group workspace): the constants cs, then xq_launch with the extraction into
// the padded rows of d_out (and d_cpy, when given). Timing goes to tenant 0's
// "linear_ggsws" bucket.
static int xq_grp_launch(fhe_group* g, const XqGrpPlan& pl, const std::vector<u64>& cs, void* ws, u64* d_out,
                         u64* d_cpy, hipStream_t st) {
  fhe_ctx* c0 = g->ctxs[0];
  const fhe_params& p = c0->p;
  int rc = store_words(c0, pl.x.at(ws).cst, cs.data(), (int64_t)cs.size(), st);
  if (rc) return rc;
  return xq_launch(
      c0, pl.x, ws, pl.total,
      [&](const XqWs& w) {
        hipLaunchKernelGGL(k_extprod_extract_grp, dim3((unsigned)pl.M, (unsigned)((p.k * p.N + 256) / 256)), dim3(256),
                           0, st, (const u64*)w.M, (const XqGrpTenant*)w.ten, (const int32_t*)w.qdt, p.N, p.k,
                           (const u64*)w.cst, d_out, d_cpy);
      },
      st);
}

int fhe_linear_ggsws_group_batch(fhe_group* g, const fhe_group_ggsw* items, int32_t T, const int64_t* const* h_cst,
                                 uint64_t* d_out, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  if (!items || T != (int32_t)g->ctxs.size()) return gfail(FHE_E_ARG, "one fhe_group_ggsw per tenant");
  if (!h_cst) return gfail(FHE_E_ARG, "null constants");
  XqGrpPlan pl;
  int rc = xq_grp_plan(g, items, T, h_cst, false, &pl);  // argument errors first
  if (rc) return rc;
  if ((rc = grp_check_params(g))) return rc;
  if (g->device < 0) return gfail(FHE_E_DEVICE, "host-only contexts");
  if (hipSetDevice(g->device) != hipSuccess) return gfail(FHE_E_DEVICE, "hipSetDevice failed");
  if (!pl.x.ns) return FHE_OK;
  if (!d_out) return gfail(FHE_E_ARG, "null output rows");
  if ((rc = grp_ensure_ws(g, pl.x.bytes))) return rc;
  const int sh = 64 - g->ctxs[0]->p.msg_bits;
  std::vector<u64> cs;
  for (int i = 0; i < pl.x.ns; ++i)
    for (int64_t q = 0; q < items[pl.tenant[i]].Q; ++q) cs.push_back((u64)h_cst[pl.tenant[i]][q] << sh);
  return xq_grp_launch(g, pl, cs, g->ws.p, d_out, nullptr, (hipStream_t)stream);
}

int fhe_search_ggsws_group_batch(fhe_group* g, const fhe_group_ggsw* items, int32_t T, void* stream) {
  if (!g) return gfail(FHE_E_ARG, "null group");
  if (!items || T != (int32_t)g->ctxs.size()) return gfail(FHE_E_ARG, "one fhe_group_ggsw per tenant");
  XqGrpPlan pl;
  int rc = xq_grp_plan(g, items, T, nullptr, true, &pl);  // argument errors first
  if (rc) return rc;
  if ((rc = grp_enter(g))) return rc;
  for (int i = 0; i < pl.x.ns; ++i) {
    const int32_t t = pl.tenant[i];
    const std::string who = "tenant " + std::to_string(t) + ": ";
    if ((rc = need_pack_key(g->ctxs[t]))) return gfail(rc, who + fhe_last_error(g->ctxs[t]));
    if (items[t].levels_bit > g->ctxs[t]->pack_key.level)
      return gfail(FHE_E_ARG, who + "levels_bit exceeds the packing key's levels");
  }
  if (!pl.x.ns) return FHE_OK;
  if ((rc = grp_ks_fits(g, pl.counts.data()))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const fhe_params& p = g->ctxs[0]->p;
  const int64_t M = pl.M;
  const size_t Wb = fhe_big_lwe_words(&p), Ws = fhe_small_lwe_words(&p), tb = grp_table_bytes((size_t)T, M);
  const size_t rows = up16(8 * (size_t)M * (3 * Wb + Ws));
  if ((rc = grp_ensure_ws(g, tb + rows + pl.x.bytes))) return rc;
  u64* small = (u64*)((char*)g->ws.p + tb);
  u64* ctv = small + (size_t)M * Ws;
  u64* sgn = ctv + (size_t)M * Wb;
  u64* cpy = sgn + (size_t)M * Wb;
  const int sh = 64 - p.msg_bits;
  std::vector<u64> cs;
  for (int i = 0; i < pl.x.ns; ++i) {
    const fhe_group_ggsw& it = items[pl.tenant[i]];
    for (int64_t q = 0; q < it.Q; ++q) cs.push_back((u64)(it.cst - it.h_T[q]) << sh);
  }
  // the leveled rows and, from the same launch, the copy the packings read
  // (the sign extraction consumes the rows)
  if ((rc = xq_grp_launch(g, pl, cs, (char*)g->ws.p + tb + rows, ctv, cpy, st))) return rc;
  if ((rc = grp_sign(g, ctv, pl.counts.data(), pl.starts.data(), M, sgn, small, g->ws.p, st))) return rc;
  // tenant t's two packings with its own key, as fhe_search_ggsws_batch
  for (int i = 0; i < pl.x.ns; ++i) {
    const int32_t t = pl.tenant[i];
    const fhe_group_ggsw& it = items[t];
    fhe_ctx* ctx = g->ctxs[t];
    if ((rc = pack_impl(ctx, cpy + (size_t)pl.starts[t] * Wb, pl.counts[t], ctx->pack_key.level, it.d_glwe_acc, st)))
      return rc;
    if ((rc = pack_impl(ctx, sgn + (size_t)pl.starts[t] * Wb, pl.counts[t],
                        it.levels_bit ? it.levels_bit : ctx->pack_key.level, it.d_glwe_bit, st)))
      return rc;
  }
  return FHE_OK;
}

}  // extern "C"

// ---- both-private key rotation: per-generation GGSW queries
// The generations' part of a call's plan: the segments are the generations
// with documents (segment -> generation), each from its first document off_g
// of the call's B; and the bridge's row map over the old ones. The workspace
// is xp_ws: XqPlan's layout, whose planes, results and constants are what
// fhe_ggsws_gens_ws_bytes counts.
struct XqGensPlan {
  XqPlan x;
  int64_t B = 0;
  int32_t gen[XQ_GENS_MAX];  // segment -> generation of the call
  int64_t off[XQ_GENS_MAX];  // generation -> its first document of the call
  int32_t n_old = 0;         // the bridge's row map: the generations before a slot -1 entry
  int64_t ends[XQ_GENS_MAX];
  int32_t slots[XQ_GENS_MAX];
};
// The argument checks of both entries (FHE_E_ARG, host-only contexts report
// them too) and the plan.
static int xq_gens_plan(fhe_ctx* ctx, const fhe_ggsw_gen* gens, int32_t G, int32_t base_log, int32_t L, int64_t Q,
                        int32_t D, XqGensPlan* pl) {
  if (!ctx) return fail(nullptr, FHE_E_ARG, "null ctx");
  if (G < 1 || G > XQ_GENS_MAX)
    return fail(ctx, FHE_E_ARG, "bad ggsw generations arguments (G outside [1, " + std::to_string(XQ_GENS_MAX) + "])");
  if (!gens) return fail(ctx, FHE_E_ARG, "null ggsw generations");
  uint32_t seen = 0;
  int64_t B = 0;
  for (int g = 0; g < G; ++g) {
    const fhe_ggsw_gen& it = gens[g];
    const std::string who = "generation " + std::to_string(g) + ": ";
    if (it.struct_size != (int32_t)sizeof(fhe_ggsw_gen))
      return fail(ctx, FHE_E_ARG, who + "fhe_ggsw_gen.struct_size is not this library's");
    if (it.slot == -1) {
      if (g != G - 1)
        return fail(ctx, FHE_E_ARG, who + "slot -1 (the current key) must be the last generation");
    } else {
      int rc = slot_arg(ctx, it.slot);
      if (rc) return rc;
      if (seen >> it.slot & 1)
        return fail(ctx, FHE_E_ARG, who + "bridge slot " + std::to_string(it.slot) + " named twice");
      seen |= 1u << it.slot;
    }
    if (it.B < 0 || it.B > 0x7fffffffLL) return fail(ctx, FHE_E_ARG, who + "B outside [0, 2^31)");
    if (it.B > 0 && (!it.d_ggsw || !it.d_docs)) return fail(ctx, FHE_E_ARG, who + "null ggsw queries or documents");
    pl->off[g] = B;
    B += it.B;
    if (it.slot != -1) {
      pl->ends[pl->n_old] = B;
      pl->slots[pl->n_old++] = it.slot;
    }
  }
  if (B < 1) return fail(ctx, FHE_E_ARG, "bad ggsw generations arguments (no generation holds a document)");
  int rc = ggsws_args(ctx, Q, B, D, base_log, L);
  if (rc) return rc;
  const fhe_params& p = ctx->p;
  pl->B = B;
  pl->x.L = L;
  const int64_t rtp = ggsws_row_tiles(p, Q, &pl->x.RT);
  for (int g = 0; g < G; ++g) {
    const fhe_ggsw_gen& it = gens[g];
    if (it.B == 0) continue;
    pl->gen[pl->x.ns] = g;
    pl->x.add(p, it.d_ggsw, it.d_docs, pl->off[g], Q, it.B, D, 0);  // one set of Q constants for all
  }
  if (!pl->x.finish(p, 0, true, Q))
    return fail(ctx, FHE_E_ARG, "ggsw queries batch too large (2^31 tiles over all generations): split the call");
  if (!FHEICP_GRP_XGENS)
    for (int i = 0; i < pl->x.ns; ++i)
      if (pl->x.seg.v[i].G > 65535 || rtp / pl->x.RT > 65535)
        return fail(ctx, FHE_E_ARG, "ggsw queries batch too large: split the call");
  return FHE_OK;
}
size_t fhe_ggsws_gens_ws_bytes(const fhe_params* p, int64_t Q, const int64_t* h_B, int32_t G, int32_t D,
                               int32_t level) {
  if (!p || !h_B || G < 1 || G > XQ_GENS_MAX || Q < 1 || D <= 0 || D > p->N || level < 1 || level > 8) return 0;
  size_t sum = 0;
  for (int g = 0; g < G; ++g) {
    if (h_B[g] < 0) return 0;
    // a generation's planes and result: the sibling's formula less the constants, which all generations share
    if (h_B[g] > 0) sum += fhe_ggsws_ws_bytes(p, Q, h_B[g], D, level) - 8 * (size_t)Q;
  }
  return sum ? sum + 8 * (size_t)Q : 0;
}
// The leveled step of every generation into d_out (Q B x (kN+1), query-major,
// generation g's documents from off_g on), h_cst[q] (or cst - h_T[q]) on query
// q's bodies: the constants, then xq_launch with the extraction by the ends
// table.
static int linear_ggsws_gens_impl(fhe_ctx* ctx, const fhe_ggsw_gen* gens, const XqGensPlan& pl, int32_t L, int64_t Q,
                                  int32_t D, const int64_t* h_cst, int64_t cst, const int64_t* h_T, uint64_t* d_out,
                                  hipStream_t st) {
  const fhe_params& p = ctx->p;
  int rc;
#if !FHEICP_GRP_XGENS
  {
    // the loop form: every generation through the single-key step into a compact buffer behind
    // the largest generation's own workspace, then scattered to its rows
    const int n1 = p.k * p.N + 1;
    size_t need = 0, rows = 0;
    for (int i = 0; i < pl.x.ns; ++i) {
      need = std::max(need, up16(fhe_ggsws_ws_bytes(&p, Q, pl.x.seg.v[i].B, D, L)));
      rows = std::max(rows, (size_t)Q * (size_t)pl.x.seg.v[i].B);
    }
    rc = reserve(ctx, ctx->xp_ws, need + 8 * rows * n1, FHE_E_DEVICE, "hipMalloc of the ggsw product workspace failed");
    if (rc) return rc;
    u64* compact = (u64*)((char*)ctx->xp_ws.p + need);
    for (int i = 0; i < pl.x.ns; ++i) {
      const XqGrpTenant& e = pl.x.seg.v[i];
      if ((rc = linear_ggsws_impl(ctx, e.ggsw, L, e.F, Q, e.B, D, h_cst, cst, h_T, compact, st))) return rc;
      hipLaunchKernelGGL(k_xq_gens_scatter, dim3((unsigned)(Q * e.B), (unsigned)((n1 + 255) / 256)), dim3(256), 0, st,
                         (const u64*)compact, (int64_t)e.B, e.start, pl.B, n1, d_out);
    }
    HIPCHK(ctx, hipGetLastError());
    return FHE_OK;
  }
#endif
  rc = reserve(ctx, ctx->xp_ws, pl.x.bytes, FHE_E_DEVICE, "hipMalloc of the ggsw product workspace failed");
  if (rc) return rc;
  void* ws = ctx->xp_ws.p;
  if ((rc = store_scaled_csts(ctx, pl.x.at(ws).cst, Q, h_cst, cst, h_T, st))) return rc;
  return xq_launch(
      ctx, pl.x, ws, Q * pl.B,
      [&](const XqWs& w) {
        hipLaunchKernelGGL(k_extprod_extract_gens, dim3((unsigned)(Q * pl.B), (unsigned)((p.k * p.N + 256) / 256)),
                           dim3(256), 0, st, (const u64*)w.M, (const XqGrpTenant*)w.ten, (const int64_t*)w.ends,
                           pl.x.ns, pl.B, p.N, p.k, (const u64*)w.cst, d_out);
      },
      st);
}

int fhe_linear_ggsws_gens_batch(fhe_ctx* ctx, const fhe_ggsw_gen* gens, int32_t G, int32_t base_log, int32_t level,
                                int64_t Q, int32_t D, const int64_t* h_cst, uint64_t* d_out, void* stream) {
  XqGensPlan pl;
  int rc = xq_gens_plan(ctx, gens, G, base_log, level, Q, D, &pl);  // argument errors first
  if (rc) return rc;
  if (!h_cst || !d_out) return fail(ctx, FHE_E_ARG, "null linear ggsw generations arguments");
  if ((rc = need_device(ctx))) return rc;
  return linear_ggsws_gens_impl(ctx, gens, pl, level, Q, D, h_cst, 0, nullptr, d_out, (hipStream_t)stream);
}

int fhe_search_ggsws_gens_batch(fhe_ctx* ctx, const fhe_ggsw_gen* gens, int32_t G, int32_t base_log, int32_t level,
                                int64_t Q, int32_t D, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                                uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream) {
  XqGensPlan pl;
  int rc = xq_gens_plan(ctx, gens, G, base_log, level, Q, D, &pl);  // argument errors first
  if (rc) return rc;
  if (levels_bit < 0 || levels_bit > 8)
    return fail(ctx, FHE_E_ARG, "bad search ggsw generations arguments (levels_bit outside [0, 8])");
  if (!h_T || !d_glwe_acc || !d_glwe_bit) return fail(ctx, FHE_E_ARG, "null search ggsw generations arguments");
  if ((rc = need_eval_keys(ctx))) return rc;
  if ((rc = need_pack_key(ctx))) return rc;
  if ((rc = gens_ready(ctx, Q, pl.B, pl.n_old, pl.ends, pl.slots))) return rc;
  if (levels_bit > ctx->pack_key.level)
    return fail(ctx, FHE_E_ARG, "search ggsw generations levels_bit exceeds the packing key's levels");
  hipStream_t st = (hipStream_t)stream;
  QueryWs w;
  if ((rc = leveled_ws(ctx, Q * pl.B, 0, true, &w, nullptr))) return rc;
  if ((rc = linear_ggsws_gens_impl(ctx, gens, pl, level, Q, D, nullptr, cst, h_T, w.ctv, st))) return rc;
  // the old generations' rows to the current key, in place; the packings' copy is taken after it
  if ((rc = bridge_gens_impl(ctx, w.ctv, Q, pl.B, pl.n_old, pl.ends, pl.slots, st))) return rc;
  return post_leveled_search(ctx, w, Q * pl.B, levels_bit, d_glwe_acc, d_glwe_bit, stream);
}
