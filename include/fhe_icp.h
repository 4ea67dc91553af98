/*
 * fhe_icp.h — C ABI of libfheicp.so, the MI355X (gfx950) engine behind the
 * encrypted pairwise compare of shipstone-labs/fhe-icp.
 *
 * Boundary. The reference reaches its hot path through a Concrete-ML
 * estimator object: FHESimilarityModel.model is a
 * concrete.ml.sklearn.LinearRegression (fhe_similarity.py:88-90) whose
 * .predict(X, fhe=...) is called at fhe_similarity.py:151 (fhe="execute",
 * encrypted), fhe_similarity.py:167 and batch_operations.py:233, :276
 * (clear). Everything BELOW that predict call (quantize -> encrypt -> leveled
 * dot product -> decrypt -> dequantize, concrete-python 2.10.0's runtime) is
 * replaced by the entry points below; the Python estimator in
 * fhe-icp_amd/fheicp/sklearn.py keeps the reference-facing API. The binding a
 * maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions.
 *  - Every function returns 0 on success and a negative FHE_E_* code on
 *    failure; fhe_last_error(ctx) (or NULL ctx) returns the message.
 *  - Pointers named d_* are DEVICE pointers on the context's device
 *    (caller-owned, e.g. torch tensors); pointers named h_* are host memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream). All
 *    launches are asynchronous on that stream unless documented otherwise.
 *  - One context per device; calls on one context must be externally
 *    serialised (same contract as the single-threaded reference callers).
 *  - Ciphertexts are little-endian u64 arrays. An LWE ciphertext of
 *    dimension d is [a_0 .. a_{d-1}, b] (d+1 words), phase = b - <a, s>
 *    modulo 2^64. "Big" ciphertexts use dimension k*N, "small" ones n.
 *  - Integer messages are encoded at Delta = 2^(64 - msg_bits).
 */
#ifndef FHE_ICP_H
#define FHE_ICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_OK 0
#define FHE_E_ARG (-1)      /* invalid argument / unsupported parameters */
#define FHE_E_DEVICE (-2)   /* HIP runtime error or no device */
#define FHE_E_STATE (-3)    /* keys not generated / imported */
#define FHE_E_NOMEM (-4)

/* Scheme parameters. After struct_size, the oracle's field
 * order (oracle/tfhe_ref.c ref_params). */
typedef struct fhe_params {
  int32_t struct_size;     /* = sizeof(fhe_params) (FHE_PARAMS_SIZE): every entry point
                              that reads a fhe_params checks it, so a binding built
                              against another version of this header (fewer or more
                              fields) fails with FHE_E_ARG instead of reading past
                              its struct or misreading fields */
  int32_t n;               /* small LWE dimension (blind-rotation length) */
  int32_t k;               /* GLWE dimension (1 or 2) */
  int32_t N;               /* polynomial size: 256, 512, 1024 or 2048 */
  int32_t pbs_base_log;    /* bootstrap gadget base log */
  int32_t pbs_level;       /* bootstrap gadget levels (1..8) */
  int32_t ks_base_log;     /* key-switch base log */
  int32_t ks_level;        /* key-switch levels */
  int32_t lwe_noise_bits;  /* TUniform bound, small LWE and KSK */
  int32_t glwe_noise_bits; /* TUniform bound, GLWE, BSK and big-key LWE */
  int32_t msg_bits;        /* P: message width of the accumulator encoding */
  int32_t sign_digit_bits; /* digit width d of fhe_sign_batch (3 or 4), or 0: the
                              widest d whose worst round keeps >= 9.2 sigma
                              (fhe_sign_digit_bits) */
  int32_t pbs_fast_base_log; /* optional second bootstrap gadget (0, 0: none). The */
  int32_t pbs_fast_level;    /* sign extraction runs its first fhe_sign_precise_rounds
                                bootstraps on (pbs_base_log, pbs_level) and the rest on
                                this cheaper one. keygen makes a second
                                bootstrapping key for it (fhe_export_fast_bsk); import
                                re-encrypts it with fresh randomness. */
  int32_t pbs_fast2_base_log; /* optional third, cheapest gadget (0, 0: none; needs the  */
  int32_t pbs_fast2_level;    /* fast one): the rounds from the plan's fast_end on use it */
  int32_t pbs_fast_group;  /* grouping factor of the fast / fast2 gadget's blind   */
  int32_t pbs_fast2_group; /* rotation: 0 or 1 = classic, one LWE coefficient per step;
                              2 = multi-bit, pairs of coefficients with three GGSWs
                              each (fhe_export_fast_bsk's layout: [pair][subset][row]
                              [component][coef]); needs N = 1024, k = 2, n <= 1023,
                              level <= 8, base_log <= 31 */
  int32_t pbs_mid_base_log;  /* optional gadgets between the main and the fast one */
  int32_t pbs_mid_level;     /* (0, 0: none; classic rotation; mid needs the fast  */
  int32_t pbs_mid2_base_log; /* gadget, mid2 needs mid): the sign plan runs the     */
  int32_t pbs_mid2_level;    /* rounds main -> mid -> mid2 -> fast -> fast2, each
                                gadget on the fewest rounds that keep every decision
                                at 9.2 sigma (fhe_sign_schedule).
                                Their keys: fhe_export_fast_bsk which = 3, 4. */
  int32_t pbs_mid_group;     /* grouping factor of the mid / mid2 gadget's blind */
  int32_t pbs_mid2_group;    /* rotation, as pbs_fast_group: 2 = multi-bit (levels
                                up to 8; 48-bit accumulators past level 2 or
                                level * base_log > 31: k_blind_rotate_mb64) */
  int32_t pbs_mid0_base_log; /* optional sixth gadget between the main and the mid */
  int32_t pbs_mid0_level;    /* one (0, 0: none; needs mid): the ladder is main ->  */
  int32_t pbs_mid0_group;    /* mid0 -> mid -> mid2 -> fast -> fast2, so a plan can run
                                its most amplified round on a multi-bit gadget as
                                precise as the classic main one (P = 26: (5,8)
                                multi-bit). Key: fhe_export_fast_bsk
                                which = 5 (stream tags 25/26, 27/28 multi-bit). */
} fhe_params;
#define FHE_PARAMS_SIZE ((int32_t)sizeof(fhe_params))

typedef struct fhe_ctx fhe_ctx;

/* ---- context -------------------------------------------------------------
 * Replaces the state Concrete builds in LinearRegression.compile()
 * (fhe_similarity.py:120: circuit + keys held on the CPU heap). device < 0
 * creates a host-only context (size queries, error strings; no kernels). */
int fhe_ctx_create(const fhe_params* params, int device, fhe_ctx** out);
void fhe_ctx_destroy(fhe_ctx* ctx);
const char* fhe_last_error(const fhe_ctx* ctx);
int fhe_get_params(const fhe_ctx* ctx, fhe_params* out);
/* Change P (msg_bits) without regenerating keys (keys do not depend on P). */
int fhe_set_msg_bits(fhe_ctx* ctx, int32_t msg_bits);

/* sizes in u64 words of the exported key material */
size_t fhe_bsk_words(const fhe_params* params);
size_t fhe_ksk_words(const fhe_params* params);
size_t fhe_big_lwe_words(const fhe_params* params);   /* k*N + 1 */
size_t fhe_small_lwe_words(const fhe_params* params); /* n + 1 */

/* ---- keys ----------------------------------------------------------------
 * Replaces Concrete keygen inside compile() (fhe_similarity.py:120) and the
 * key material FHEKeyManager.generate_keys means to persist
 * (key_management.py:112-191). Every key word is a ChaCha20 stream word
 *  under a 256-bit key. fhe_keygen_key is the production entry:
 * pass 32 bytes from the OS CSPRNG. fhe_keygen expands a 64-bit seed by
 * splitmix64 — 64 bits of entropy, NOT for production keys: reproducible
 * tests, fixtures and benches only. */
int fhe_keygen_key(fhe_ctx* ctx, const uint32_t h_key[8], void* stream);
int fhe_keygen(fhe_ctx* ctx, uint64_t seed, void* stream);
/* Host copies of the canonical key material; any pointer may be NULL.
 * s_small: n words (0/1); s_big: k*N words (0/1); bsk: fhe_bsk_words
 * (coefficient domain, [i][row][component][coef]); ksk: fhe_ksk_words
 * ([i][level][n+1]). Synchronous. */
int fhe_export_keys(fhe_ctx* ctx, uint64_t* h_s_small, uint64_t* h_s_big, uint64_t* h_bsk, uint64_t* h_ksk);
int fhe_import_keys(fhe_ctx* ctx, const uint64_t* h_s_small, const uint64_t* h_s_big, const uint64_t* h_bsk,
                    const uint64_t* h_ksk);
/* a fast gadget's bootstrapping key, which = 1 (pbs_fast_*, stream tags
 * 9/10, or 13/14 for a multi-bit key), 2 (pbs_fast2_*, tags 11/12 or
 * 15/16), 3 (pbs_mid_*, tags 17/18), 4 (pbs_mid2_*, tags 19/20) or 5
 * (pbs_mid0_*, tags 25/26; 21/22, 23/24 and 27/28 multi-bit): the
 * layout of bsk with one GGSW per LWE coefficient, or three per
 * pair of coefficients ([pair][subset {1}, {2}, {1,2}][row][component][coef])
 * when that gadget's group is 2; fhe_fast_bsk_words words (0: no such
 * gadget). FHE_E_STATE without that gadget. Synchronous. */
size_t fhe_fast_bsk_words(const fhe_params* params, int32_t which);
int fhe_export_fast_bsk(fhe_ctx* ctx, int32_t which, uint64_t* h_bsk);
/* Evaluation keys only: bsk, ksk and every present gadget's key
 * (h_gadget_bsk[g - 1] in fhe_export_fast_bsk's layout for which = g; ignored
 * for absent gadgets, FHE_E_ARG when a present one is missing). The keys are
 * used as given, nothing is re-encrypted. The context then holds no secret
 * key (one it held is zeroed and freed): the encrypting, decrypting, compare,
 * score and sign-trace entry points, fhe_keygen_pack_key and fhe_export_keys
 * with a secret pointer return FHE_E_STATE; the leveled, key-switch,
 * bootstrap, sign, threshold, query, top-k, pack and search entry points and
 * fhe_export_keys(NULL, NULL, bsk, ksk) / fhe_export_fast_bsk work.
 * Synchronous. */
int fhe_import_eval_keys(fhe_ctx* ctx, const uint64_t* h_bsk, const uint64_t* h_ksk,
                         const uint64_t* const h_gadget_bsk[5]);

/* ---- client side: encrypt / decrypt --------------------------------------
 * Replaces the per-sample encrypt/decrypt of predict(fhe="execute")
 * (fhe_similarity.py:151). Ciphertext c uses stream id (id0 + c).
 * Encryption randomness. Every encrypting entry point comes in two forms:
 * `*_key` takes the 256-bit ChaCha20 stream key (h_key / h_enc_key, 8 words),
 * the production form — one fresh CSPRNG key per session, independent of the
 * secret key's, with a random 64-bit id0 start, and stream ids (id0 + ...)
 * never reused under one key; the plain form takes a 64-bit `seed`
 * expanded by splitmix64 (fhe_key_from_seed): tests and benches only. */
int fhe_encrypt_batch_key(fhe_ctx* ctx, const int64_t* d_msg, int64_t count, const uint32_t h_key[8], uint64_t id0,
                          uint64_t* d_ct, void* stream);
int fhe_encrypt_batch(fhe_ctx* ctx, const int64_t* d_msg, int64_t count, uint64_t seed, uint64_t id0,
                      uint64_t* d_ct, void* stream);
/* round(phase / Delta) as signed msg_bits-bit integers */
int fhe_decrypt_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int64_t* d_out, void* stream);
/* 1 iff phase is nearer 2^63 than 0 (decrypts a sign/bit ciphertext) */
int fhe_decrypt_bits_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int64_t* d_out, void* stream);
/* raw phases (tests / noise measurement) */
int fhe_phase_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, uint64_t* d_out, void* stream);

/* ---- server side -----------------------------------------------------------
 * The leveled circuit of Concrete-ML LinearRegression._inference:
 *   out[b] = sum_j d_w[j] * ct[b, j] + trivial(cst * Delta),
 * ct: B x D big ciphertexts (row-major), d_w: D int64 (device). */
int fhe_linear_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                     uint64_t* d_out, void* stream);
/* Packed feature encryption, the client side of the
 * reference's predict(fhe="execute") (fhe_similarity.py:151): the D features
 * of row b (d_qx, B x D, encoded at Delta) are the first coefficients of
 * G = ceil(D / N) GLWE messages; GLWE (b, g) uses stream id id0 + b*G + g.
 * d_glwe: B x G x (k+1)N words [A_1 .. A_k, B] per GLWE. */
int fhe_encrypt_packed_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const uint32_t h_key[8],
                                 uint64_t id0, uint64_t* d_glwe, void* stream);
int fhe_encrypt_packed_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, uint64_t seed, uint64_t id0,
                             uint64_t* d_glwe, void* stream);
/* The leveled dot product on packed inputs (Concrete-ML
 * LinearRegression._inference's q_x @ q_w + constant): out[b] = sum_g
 * SampleExtract_0(GLWE(b, g) * sum_t d_w[gN + t] X^-t) + trivial(cst * Delta),
 * a big LWE (B x (kN+1)) of sum_j d_w[j] x[b, j] + cst. Needs no secret key. */
int fhe_linear_packed_batch(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t B, int32_t D, const int64_t* d_w,
                            int64_t cst, uint64_t* d_out, void* stream);
/* fhe_encrypt_packed_batch followed by fhe_linear_packed_batch, fused: the
 * GLWEs are never written (bit-identical to the two calls). The single-party
 * form of predict(fhe="execute"): client encryption and the server's leveled
 * dot product in one pass; d_out: B x (kN+1). */
int fhe_encrypt_linear_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const uint32_t h_key[8],
                                 uint64_t id0, const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream);
int fhe_encrypt_linear_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, uint64_t seed, uint64_t id0,
                             const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream);
/* big -> small key switch of (ct << shift) + add_body (shift/add used by the
 * bit extraction; pass 0, 0 for a plain key switch) */
int fhe_keyswitch_batch(fhe_ctx* ctx, const uint64_t* d_big, int64_t count, int32_t shift, uint64_t add_body,
                        uint64_t* d_small, void* stream);
/* Programmable bootstrap with the constant test vector `tv` (output phase
 * ~ +tv if the input phase is in [0, 2^63), ~ -tv otherwise), sample-
 * extracted under the big key. d_small: count x (n+1); d_out: count x (kN+1). */
int fhe_pbs_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, uint64_t tv, uint64_t* d_out,
                  void* stream);
/* fhe_pbs_batch on one of the parameter set's gadgets: 0 = the main one
 * (pbs_base_log, pbs_level), 1 = pbs_fast_*, 2 = pbs_fast2_*, 3 = pbs_mid_*,
 * 4 = pbs_mid2_*, 5 = pbs_mid0_* (with their own
 * bootstrapping keys and kernels, e.g. the multi-bit rotation of
 * pbs_fast_group = 2). FHE_E_STATE if that gadget is
 * absent. */
int fhe_pbs_gadget_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, int32_t gadget, uint64_t tv,
                         uint64_t* d_out, void* stream);
/* Exact LSB-first bit extraction of the msg_bits-bit value v encrypted in
 * d_ct_v (consumed). d_refreshed receives a fresh encryption of v (sum of
 * the bit ciphertexts), d_sign the ciphertext of the top bit ([v < 0] at
 * 2^63). msg_bits key-switches and bootstraps per ciphertext. */
int fhe_bit_extract_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_refreshed, uint64_t* d_sign,
                          void* stream);

/* Sign of the msg_bits-bit value v in d_ct_v (consumed): d_sign receives the
 * encryption of [v < 0] at 2^63 (decrypt with fhe_decrypt_bits_batch). Uses
 * fhe_sign_pbs_count(params) key switches + bootstraps per ciphertext: d-bit
 * digits (d = fhe_sign_digit_bits), two bootstraps each, then the sign of the
 * top d bits; 7 at msg_bits = 16 (d = 4). */
int fhe_sign_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, uint64_t* d_sign, void* stream);
/* Resolved digit width (params->sign_digit_bits, or the noise-model choice
 * when it is 0); 0 for msg_bits < 4 (single-bit rounds); -1 on bad params. */
int fhe_sign_digit_bits(const fhe_params* params);
int fhe_sign_pbs_count(const fhe_params* params);
/* how many of them (the first ones) run on the main gadget; all of them
 * without a fast gadget */
int fhe_sign_precise_rounds(const fhe_params* params);
/* the whole plan: digit width, bootstraps [0, main_rounds) on the main
 * gadget, [main_rounds, fast_end) on the mid0, mid, mid2 and fast ones (in
 * that order, fhe_sign_schedule), the rest on fast2
 * (DESIGN.md §3.6). Any pointer may be NULL. */
int fhe_sign_plan(const fhe_params* params, int32_t* digit_bits, int32_t* main_rounds, int32_t* fast_end);
/* the gadget (0..5, as fhe_pbs_gadget_batch) of every bootstrap of
 * fhe_sign_batch in order, into gadgets[0 .. min(R, cap)); returns R (the
 * bootstraps per sign extraction) or FHE_E_ARG on bad params. */
int fhe_sign_schedule(const fhe_params* params, int32_t* gadgets, int32_t cap);
/* MEASUREMENT ONLY (reads the secret key; no reference counterpart): the
 * decision noise behind the exactness of fhe_sign_batch (the decision of
 * batch_operations.py:278). Runs fhe_sign_batch's rounds on one stream, with
 *  - h_sched (host, R entries, NULL = fhe_sign_schedule's plan): the gadget
 *    of every round, e.g. a deliberately noisier one to narrow a margin;
 *  - rounds: stop after the first `rounds` bootstraps (0 = all R); d_sign is
 *    written (and required) only when the last round runs;
 *  - d_phase (device, NULL = none): round r's rotation exponent for
 *    ciphertext c at d_phase[r * count + c], the bootstrap input's phase
 *    modulus-switched to 2N exactly as that round's rotation (classic or
 *    multi-bit) rounds it, i.e. the test-vector index the rotation selects.
 * tests/test_gpu_decision_noise.py compares these with the exact rounds. */
int fhe_sign_trace_batch(fhe_ctx* ctx, uint64_t* d_ct_v, int64_t count, const int32_t* h_sched, int32_t rounds,
                         uint64_t* d_sign, uint32_t* d_phase, void* stream);
/* Bootstrap with a staircase test vector over 2^log_slots slots of the half
 * torus: output phase ~ base + floor(phase * 2^log_slots / 2^63) * step for an
 * input phase in [0, 2^63) (negacyclic beyond). log_slots = 0, step = 0 is
 * fhe_pbs_batch with tv = base. */
int fhe_pbs_lut_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, uint64_t base, uint64_t step,
                      int32_t log_slots, uint64_t* d_out, void* stream);

/* Programmable bootstrap with an arbitrary table (SURVEY.md §8b
 * fhe_pbs_batch(ctx, ct_in, B, const int64* lut, ct_out)): the input small
 * LWE encrypts a message m in [0, 2^lut_bits) at 2^(63 - lut_bits) (one
 * padding bit); the output big LWE encrypts d_lut[m] (a signed msg_bits-bit
 * value) at Delta = 2^(64 - msg_bits). The test vector is built on the device
 * from d_lut (2^lut_bits int64, device memory): box m covers the input phases
 * within half a box of m * 2^(63 - lut_bits). 0 <= lut_bits <= log2(N) - 1;
 * the caller keeps the input noise (after key and modulus switching) inside
 * half a box. */
int fhe_pbs_table_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, const int64_t* d_lut, int32_t lut_bits,
                        uint64_t* d_out, void* stream);
/* fhe_pbs_table_batch on an explicit gadget (0..5, as fhe_pbs_gadget_batch):
 * a multi-bit gadget runs the sign extraction's multi-bit rotation
 * (k_blind_rotate_mb / _mb64) with the table test vector and that gadget's
 * key; 0 the classic main gadget. fhe_pbs_table_batch takes
 * fhe_pbs_table_gadget(params): the most precise multi-bit gadget of the set
 * (smallest bootstrap noise), 0 when it has none; FHE_E_ARG on bad params. */
int fhe_pbs_table_gadget_batch(fhe_ctx* ctx, const uint64_t* d_small, int64_t count, int32_t gadget,
                               const int64_t* d_lut, int32_t lut_bits, uint64_t* d_out, void* stream);
int fhe_pbs_table_gadget(const fhe_params* params);
/* The encrypted decision of batch_operations.py:278 (score >= min_similarity
 * <=> acc >= T, SURVEY.md §8b fhe_threshold_batch): d_ct_acc holds big LWEs of
 * msg_bits-bit accumulators (not modified); d_bit receives the encryption of
 * [acc >= T] at 2^63 (fhe_decrypt_bits_batch). acc - T must fit msg_bits
 * bits. fhe_sign_pbs_count(params) key switches + bootstraps per ciphertext. */
int fhe_threshold_batch(fhe_ctx* ctx, const uint64_t* d_ct_acc, int64_t count, int64_t T, uint64_t* d_bit,
                        void* stream);

/* ---- fused compare / search ------------------------------------------------
 * One call per batch of B (query, document) pairs — the batched replacement
 * of the per-document loop at batch_operations.py:268-279 and of
 * compare_encrypted (batch_operations.py:206-238):
 *   encrypt q_x (B x D) -> linear with d_w and cst - T -> decrypt the
 *   leveled accumulator -> sign extraction (fhe_sign_pbs_count(params)
 *   KS + PBS) -> decrypt the sign bit. d_acc[b] = the decrypted accumulator (exact int64, = Concrete's
 *   q_x @ q_w - zp*sum(q_w) + q_b; read from the leveled ciphertext like the
 *   reference's leveled circuit), d_below[b] = 1 iff acc < T (the decrypted
 *   bootstrapped threshold bit; acc >= T <=> score >= min_similarity).
 * Uses context-owned workspace of ~8 * B * (2(kN+1) + n + 2) bytes (grown on
 * demand; not graph-capturable): the encryption is fused into the linear step
 * (fhe_encrypt_linear_batch), so D does not enter the footprint. The `_key`
 * form takes the session's 256-bit encryption key (see "Encryption
 * randomness"); the enc_seed form is for tests and benches. */
int fhe_compare_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                          int64_t T, const uint32_t h_enc_key[8], uint64_t id0, int64_t* d_acc, int64_t* d_below,
                          void* stream);
int fhe_compare_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                      int64_t T, uint64_t enc_seed, uint64_t id0, int64_t* d_acc, int64_t* d_below, void* stream);
/* The reference's predict(fhe="execute") as it is (fhe_similarity.py:142-160,
 * one row per call at :149-158): a leveled circuit with no PBS. encrypt q_x
 * -> linear with d_w and cst - T -> decrypt; d_acc[b] = the accumulator
 * (exact int64). No key switch or bootstrap runs; T only centres the value in
 * the msg_bits-bit encoding (acc - T must fit it; the estimator passes the
 * middle of the accumulator range). Workspace ~8 * B * (kN + 2) bytes.
 * `_key` form: the session's 256-bit encryption key, as fhe_compare_batch_key. */
int fhe_score_batch_key(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                        int64_t T, const uint32_t h_enc_key[8], uint64_t id0, int64_t* d_acc, void* stream);
int fhe_score_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D, const int64_t* d_w, int64_t cst,
                    int64_t T, uint64_t enc_seed, uint64_t id0, int64_t* d_acc, void* stream);

/* ---- seeded (compressed) ciphertexts: the encrypted document corpus -------
 * Persisted documents (EncryptedDocument at
 * encrypted_storage.py:19-51, whose `encrypted_embedding` is a plaintext
 * vector in the reference, batch_operations.py:175-178) are stored as
 * seeded LWEs: only the body word per feature. The mask of feature j of
 * document b is ChaCha20 stream (TAG_ENC_MASK, id0[b] + j) under the PUBLIC
 * 256-bit mask key; the noise comes from the SECRET noise key. A corpus in
 * HBM is then B x D body words plus B ids instead of B x D x (kN + 1) words;
 * the masks are regenerated inside the kernels that consume them.
 * d_msg / d_body: B x D (row-major), d_id0: B u64 (stream ids must not repeat
 * under one mask key). */
int fhe_encrypt_seeded_batch(fhe_ctx* ctx, const int64_t* d_msg, int64_t B, int32_t D, const uint32_t h_mask_key[8],
                             const uint32_t h_noise_key[8], const uint64_t* d_id0, uint64_t* d_body, void* stream);
/* full ciphertexts (B*D x (kN+1)) of a seeded corpus; needs no secret key */
int fhe_expand_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                            const uint32_t h_mask_key[8], uint64_t* d_ct, void* stream);
/* fhe_linear_batch on a seeded corpus (masks regenerated in registers):
 * out[b] = sum_j d_w[j] * ct(b, j) + trivial(cst * Delta); B x (kN+1). */
int fhe_linear_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                            const uint32_t h_mask_key[8], const int64_t* d_w, int64_t cst, uint64_t* d_out,
                            void* stream);
/* fhe_compare_batch over a stored encrypted corpus: linear (seeded) with d_w
 * and cst - T -> decrypt the leveled accumulator -> sign extraction ->
 * decrypt the threshold bit. The documents were encrypted at some P0 >= the
 * context's msg_bits P; the caller folds 2^(P0 - P) into d_w. */
int fhe_compare_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                             const uint32_t h_mask_key[8], const int64_t* d_w, int64_t cst, int64_t T,
                             int64_t* d_acc, int64_t* d_below, void* stream);
/* ---- private-query search: an encrypted query against clear documents -----
 * The third deployment shape: the store keeps plaintext
 * embeddings, as the reference's does (batch_operations.py:175-178), and the
 * QUERY arrives encrypted. Query and documents are quantized by one symmetric
 * n_e <= 8 bit quantizer; the server holds the quantized documents dq (B x D)
 * in the clear and computes
 *   out[b] = sum_j dq[b, j] * (d_w[j] * ct_q[j]) + trivial(cst * Delta),
 * an integer GEMM [B x D] . [D x (kN+1)] over Z_2^64 on the i8 matrix cores,
 * bit-identical to the plain u64 sum.
 * fhe_query_docs_pack turns dq (int64, values in [-128, 127]) into the GEMM's
 * document operand, once per resident corpus: fhe_query_docs_bytes bytes
 * (B padded to a multiple of 16, D to a multiple of 64; one byte each).
 * Document group i (rows 16 i .. 16 i + 15) occupies bytes [i, i + 1) * 16 *
 * padded D, so a batch that starts at a multiple of 16 documents is a pointer
 * into d_docs8.
 * 0 < D <= 65536 (the i32 accumulators); d_w may hold any 64-bit weights. */
size_t fhe_query_docs_bytes(const fhe_params* params, int64_t B, int32_t D);
int fhe_query_docs_pack(fhe_ctx* ctx, const int64_t* d_dq, int64_t B, int32_t D, void* d_docs8, void* stream);
/* The leveled step alone: d_ct_q holds the query's D full ciphertexts
 * (D x (kN+1)), d_out B x (kN+1). Needs no keys. The query's byte planes live
 * in context-owned workspace (8 * 64 ceil(D/64) * 16 ceil((kN+1)/16) bytes,
 * grown on demand). */
int fhe_linear_query_batch(fhe_ctx* ctx, const uint64_t* d_ct_q, const void* d_docs8, int64_t B, int32_t D,
                           const int64_t* d_w, int64_t cst, uint64_t* d_out, void* stream);
/* fhe_compare_seeded_batch with the roles swapped. The query travels as a
 * seeded LWE vector (fhe_encrypt_seeded_batch with B = 1): D body words
 * (d_qbody, device), its stream id id0 (feature j under id0 + j) and the
 * public mask key. Expand the query -> planes -> GEMM with d_w and cst - T ->
 * decrypt the leveled accumulator -> sign extraction -> decrypt the threshold
 * bit. The query was encrypted at the context's msg_bits. Same single-party
 * contract and outputs as fhe_compare_seeded_batch: d_acc[b] the accumulator,
 * d_below[b] = 1 iff acc < T. */
int fhe_compare_query_batch(fhe_ctx* ctx, const uint64_t* d_qbody, uint64_t id0, const uint32_t h_mask_key[8],
                            const void* d_docs8, int64_t B, int32_t D, const int64_t* d_w, int64_t cst, int64_t T,
                            int64_t* d_acc, int64_t* d_below, void* stream);

/* ---- two-party private query: packed GLWE replies --------
 * A server that holds evaluation keys only (fhe_import_eval_keys) cannot
 * decrypt in place; it folds up to N result LWEs into one GLWE under the big
 * key with a packing key switch and returns (k+1)N words per N results.
 * All arithmetic modulo 2^64. The gadget (base_log b, level L), 1 <= b <= 7,
 * 1 <= L <= 8, L (b + 1) <= 62, is an argument, not a field of fhe_params.
 * Packing key row (i, l), i < kN, l = 1..L: a GLWE encryption under the big
 * key read as k polynomials (S_c[t] = s_big[cN + t]) of the constant
 * polynomial s_big[i] * 2^(64 - b l), noise TUniform(glwe_noise_bits), stream
 * tags 29/30; layout [i][l][component 0..k][coef], fhe_pack_key_words words
 * (0 for a gadget out of range). For big LWEs (a_j, b_j), j < count <= N:
 *   out = sum_j X^j [ (0, .., 0, b_j) - sum_i sum_{l <= L'} d_{j,i,l} PK[i][l] ]
 * negacyclic in X, d_{j,i,.} the key switch's balanced digits with tie coins
 * of a_{j,i} on L' <= L levels. Coefficient j of the phase B - sum_c A_c S_c
 * is LWE j's phase plus rounding and key noise; for count > N, GLWE g packs
 * inputs gN .. gN + N - 1; coefficients past count carry noise only. */
size_t fhe_pack_key_words(const fhe_params* params, int32_t base_log, int32_t level);
/* Generate the context's packing key (needs the secret key; replaces any
 * earlier one). `*_key` / seed forms as for the encrypting entry points. */
int fhe_keygen_pack_key_key(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_key[8], void* stream);
int fhe_keygen_pack_key(fhe_ctx* ctx, int32_t base_log, int32_t level, uint64_t seed, void* stream);
/* Host copy of the packing key / install one (converted once to byte planes
 * for the i8 matrix cores). Import needs no other key. Synchronous. */
int fhe_export_pack_key(fhe_ctx* ctx, uint64_t* h_out);
int fhe_import_pack_key(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint64_t* h_in);
/* Pack count big LWEs (count x (kN+1)) into ceil(count / N) GLWEs
 * (d_glwe: each (k+1)N words [A_1 .. A_k, B]) on the first `levels` levels of
 * the key (0: all). Needs only the packing key. Bit-exact. */
int fhe_pack_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, int32_t levels, uint64_t* d_glwe, void* stream);
/* Decrypt the first `count` coefficients of packed GLWEs: mode 0 signed
 * msg_bits-bit values (as fhe_decrypt_batch), 1 bits (fhe_decrypt_bits_batch),
 * 2 raw phases (fhe_phase_batch). Needs the secret key. */
int fhe_decrypt_packed_batch(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t count, int32_t mode, int64_t* d_out,
                             void* stream);
/* The cheapest gadget (fewest levels, then the largest base_log <= 7) with
 *   2^(63 - msg_bits) / sqrt(in_var 2^128 + var_pack) >= 9.2,
 *   var_pack = min(count, N) kN L ((B^2 + 2) / 12) tuniform_var(glwe_noise_bits)
 *              + (1 + kN / 2) 2^(2 (64 - b L)) / 12,   B = 2^b,
 * in_var the inputs' variance in torus units; bit_levels the shortest level
 * prefix that keeps 9.2 sigma for a bit at 2^63 (margin 2^62). When no gadget
 * reaches the bar, the most precise one (the caller reports the margin).
 * Host only; fheicp.params.pack_plan is the same function. */
int fhe_pack_plan(const fhe_params* params, int64_t count, double in_var, int32_t* base_log, int32_t* level,
                  int32_t* bit_levels);
/* The server entry: fhe_compare_query_batch's pipeline without either
 * decryption. Expand the query -> planes -> GEMM with cst - T -> copy of the
 * leveled ciphertexts -> sign extraction -> pack the copies into d_glwe_acc
 * (all levels) and the sign ciphertexts into d_glwe_bit (the first levels_bit
 * levels, 0: all); each ceil(B / N) x (k+1)N words. Needs evaluation keys and
 * the packing key, no secret. The client decrypts d_glwe_acc with mode 0 and
 * adds T, and d_glwe_bit with mode 1 (= below). */
int fhe_search_query_batch(fhe_ctx* ctx, const uint64_t* d_qbody, uint64_t id0, const uint32_t h_mask_key[8],
                           const void* d_docs8, int64_t B, int32_t D, const int64_t* d_w, int64_t cst, int64_t T,
                           int32_t levels_bit, uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream);
/* ---- both-private search: GGSW query x GLWE documents -----
 * The fourth deployment shape: the host sees neither the documents nor the
 * query. Everything is exact arithmetic modulo 2^64 on the i8 matrix cores.
 * Documents: S = floor(N / D) documents share one GLWE under the big key,
 * feature j of document i at coefficient i D + j, encoded at Delta =
 * 2^(64 - msg_bits): fhe_encrypt_packed_batch on rows of S D values (unused
 * coefficients 0), G = ceil(B / S) GLWEs per B documents. D <= N.
 * Query: the client forms W_j = q_w[j] qq_j (plain integers) and sends one
 * GGSW of Q = sum_j W_j X^-j under the big key with gadget (base_log b,
 * level L; the packing gadget's bounds): row (c, l), c <= k, l = 1..L, is a
 * GLWE encryption of Q 2^(64 - b l) for c = k and of -S_c Q 2^(64 - b l) for
 * c < k, noise TUniform(glwe_noise_bits), stream tags 31/32 (row r = c L +
 * (l - 1): masks from stream id0 + r k + component, noise from id0 + r; a
 * GGSW consumes ids id0 .. id0 + (k+1) L k - 1). Layout
 * [c][l][component 0..k][coef], fhe_ggsw_words words (0 for a gadget out of
 * range). The encrypting entries need the secret key: FHE_E_DEVICE on a
 * host-only context, FHE_E_STATE on an evaluation-only one. `*_key` / seed
 * forms as for the other encrypting entry points. d_w: D int64 (device). */
size_t fhe_ggsw_words(const fhe_params* params, int32_t base_log, int32_t level);
int fhe_encrypt_ggsw_key(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t base_log, int32_t level,
                         const uint32_t h_key[8], uint64_t id0, uint64_t* d_ggsw, void* stream);
int fhe_encrypt_ggsw(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t base_log, int32_t level, uint64_t seed,
                     uint64_t id0, uint64_t* d_ggsw, void* stream);
/* The cheapest gadget (fewest levels, then the largest base_log <= 7; level
 * <= 8, level (base_log + 1) <= 62) with 2^(63 - msg_bits) / sqrt(var) >= 9.2,
 *   var = w_norm2 tv + (k+1) L N ((B^2 + 2) / 12) tv
 *         + w_norm2 (1 + kN / 2) 2^(2 (64 - b L)) / 12,
 * tv = tuniform_var(glwe_noise_bits), B = 2^b, w_norm2 the worst-case
 * sum_j W_j^2 (4^(n_e - 1) sum_j q_w[j]^2). FHE_E_STATE (outputs 0) when no
 * gadget reaches the bar. Host only; fheicp.params.extprod_plan is the same. */
int fhe_extprod_plan(const fhe_params* params, double w_norm2, int32_t* base_log, int32_t* level);
/* The documents' digits as the GEMM's left operand, once per resident corpus:
 * d_glwe holds the G = ceil(B / floor(N / D)) document GLWEs, d_docs8 receives
 * fhe_glwe_docs_bytes bytes (G padded to a multiple of 16, one byte per word
 * and level; 0 for bad arguments). Needs no keys. */
size_t fhe_glwe_docs_bytes(const fhe_params* params, int64_t B, int32_t D, int32_t level);
int fhe_glwe_docs_pack(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t B, int32_t D, int32_t base_log, int32_t level,
                       void* d_docs8, void* stream);
/* The leveled step: with d_{c,.} the key switch's balanced digits with tie
 * coins of component c (masks and body alike) of a document GLWE,
 *   out = sum_{c <= k} sum_{l <= L} d_{c,l}(X) Row(c, l)   (negacyclic, mod 2^64),
 * coefficient i D of whose phase is sum_j W_j dq[i, j] Delta plus noise; that
 * coefficient is sample-extracted and trivial(cst Delta) added: d_out is
 * B x (kN+1), what fhe_sign_batch and fhe_pack_batch take. Bit-exact. Needs
 * no keys. The query's negacyclic Toeplitz byte planes (8 ((k+1)N)^2 L bytes:
 * 528 MB at N = 1024, k = 2, L = 7) live in context-owned workspace allocated
 * on first use. (base_log, level) are the query's and the packed digits'. */
int fhe_linear_ggsw_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs8,
                          int64_t B, int32_t D, int64_t cst, uint64_t* d_out, void* stream);
/* fhe_compare_query_batch with both sides encrypted (single party: decrypts):
 * leveled step with cst - T -> decrypt the accumulator -> sign extraction ->
 * decrypt the threshold bit. Same outputs as fhe_compare_query_batch. */
int fhe_compare_ggsw_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs8,
                           int64_t B, int32_t D, int64_t cst, int64_t T, int64_t* d_acc, int64_t* d_below,
                           void* stream);
/* The untrusted host's entry: fhe_search_query_batch with both sides
 * encrypted. Evaluation keys and the packing key only; replies as there. */
int fhe_search_ggsw_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs8,
                          int64_t B, int32_t D, int64_t cst, int64_t T, int32_t levels_bit, uint64_t* d_glwe_acc,
                          uint64_t* d_glwe_bit, void* stream);
/* The 64-bit-seed -> 256-bit ChaCha key expansion used by the seed forms
 * (fhe_keygen, fhe_encrypt_batch, ...; splitmix64): tests and
 * benches only. Host only. */
void fhe_key_from_seed(uint64_t seed, uint32_t h_key_out[8]);

/* ---- clear pre/post-processing on the device ----------------------------
 * Pair features and Concrete-ML's input quantizer in one pass:
 * X[b, j] = query[j] * docs[b, j] in numpy's promoted dtype (the query may be
 * f64, batch_operations.py:260; stored docs are f32, :178), or X = docs when
 * d_query is NULL; then q = clip(rint(X / scale + zero_point), qmin, qmax)
 * in float64 (concrete-ml UniformQuantizer.quant). Bit-identical to numpy. */
int fhe_quantize_pairs(fhe_ctx* ctx, const void* d_query, int32_t query_is_f64, const void* d_docs,
                       int32_t docs_is_f64, int64_t B, int32_t D, double scale, int64_t zero_point, int64_t qmin,
                       int64_t qmax, int64_t* d_qx, void* stream);
/* The embedding stage's PCA (dimension_reduction.py:67-72: sklearn
 * PCA.transform, no whitening), SURVEY.md §8f-4: d_out[b][d] = sum_k
 * (d_x[b][k] - d_mean[k]) * d_components[d][k] for B rows of K <= 1024
 * float32 features and D components (row-major, as PCA.components_),
 * accumulated in f64 and stored as float32 (the reference stores float32
 * embeddings, batch_operations.py:175-178). Needs no keys. */
int fhe_pca_transform(fhe_ctx* ctx, const float* d_x, int64_t B, int32_t K, const float* d_mean,
                      const float* d_components, int32_t D, float* d_out, void* stream);
/* score[b] = out_scale * (double)acc[b] (UniformQuantizer.dequant, zp 0) */
int fhe_dequantize(fhe_ctx* ctx, const int64_t* d_acc, int64_t B, double out_scale, double* d_score, void* stream);

/* Top-k of d_acc over entries with d_below == 0 (or all if d_below is
 * NULL), ordered by (acc desc, index asc) — Python's stable sort of
 * batch_operations.py:282 on a monotone dequantisation. Indices are
 * base_idx + position. Missing slots get acc = INT64_MIN, idx = -1. */
int fhe_topk(fhe_ctx* ctx, const int64_t* d_acc, const int64_t* d_below, int64_t B, int64_t base_idx, int32_t k,
             int64_t* d_out_acc, int64_t* d_out_idx, void* stream);

/* ---- device memory -------------------------------------------------------
 * For callers without a device allocator of their own (a ctypes binding from
 * numpy); torch callers pass tensor pointers instead.
 * fhe_memcpy_d2h returns after the copy completed (it synchronises `stream`). */
int fhe_dev_alloc(fhe_ctx* ctx, size_t bytes, void** d_out);
int fhe_dev_free(fhe_ctx* ctx, void* d_ptr);
int fhe_memcpy_h2d(fhe_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream);
int fhe_memcpy_d2h(fhe_ctx* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream);
int fhe_stream_sync(fhe_ctx* ctx, void* stream);

/* ---- measurement ------------------------------------------------------------
 * When enabled, every blind-rotation (external-product) and key-switch
 * launch is bracketed by hipEvents on its own stream. fhe_profile_read
 * synchronises and returns total milliseconds, launch count and ciphertexts
 * processed for kernel "blind_rotate" (all gadgets), "blind_rotate_main",
 * "blind_rotate_fast" (fhe_params.pbs_fast_*), "blind_rotate_fast2",
 * "blind_rotate_mid", "blind_rotate_mid2", "blind_rotate_mid0", "keyswitch", "encrypt_linear"
 * (the fused client encryption + leveled dot), "linear_query" (the
 * private-query leveled step: query planes + GEMM, one bracket around both)
 * "pack" (the packing key switch: digits + GEMM + rotation, one bracket),
 * "bridge" (the bridge key switch of rotated documents: digits + GEMM +
 * scatter, one bracket),
 * "linear_ggsw" (the both-private leveled step: Toeplitz planes + GEMM +
 * slot extraction, one bracket), "linear_ggsws" (the same step of the batched
 * entries: GGSW byte planes + the transposed GEMM + slot extraction) or
 * "linear_seeded" (the stored-ciphertext leveled step of the batched entries,
 * k_linear_seeded_queries), then resets what it read. */
int fhe_profile_enable(fhe_ctx* ctx, int enable);
int fhe_profile_read(fhe_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches, int64_t* items);
/* The kernel last launched for that bucket, as rocprofv3 names it (e.g.
 * "k_blind_rotate_v4<2, true, 0, 4, false, 15>", "k_blind_rotate_mb<1, 0, 23>",
 * "k_keyswitch_mfma"); "" before any launch. Not reset by fhe_profile_read. */
int fhe_profile_kernel_name(fhe_ctx* ctx, const char* kernel, char* h_buf, size_t len);
/* "libfheicp gfx950 ab=0" for the shipped build; ab=1 for A/B builds
 * (tools/build_variant.sh -DFHEICP_AB: extra v4 shapes, v3, timing kernels). */
const char* fhe_build_info(void);

/* ---- private-query search: several queries in one pass ----
 * Q encrypted queries of ONE key holder (one context, one set of evaluation
 * keys, one mask key) against the same B packed documents: one leveled GEMM
 * launch, one sign extraction over Q * B ciphertexts, one packing. Results
 * are query-major: result (q, b) is row / element q * B + b. Q >= 1, B >= 1,
 * 0 < D <= 65536, Q <= 65535; bad arguments return FHE_E_ARG, missing keys
 * FHE_E_STATE, as in the single-query entries. The stream ids of one batch
 * must not overlap: id ranges [id0_q, id0_q + D) are disjoint modulo 2^64
 * (no id repeats under one mask key).
 *
 * The leveled step alone: d_ct_q holds Q * D full ciphertexts ([Q][D][kN+1]),
 * h_cst Q host constants (one per query), d_out Q * B x (kN+1) with
 *   out[q B + b] = sum_j dq[b][j] * (d_w[j] * ct_q[q][j]) + trivial(h_cst[q] * Delta),
 * word for word what Q calls of fhe_linear_query_batch write. Needs no keys.
 * The plane workspace grows to Q times the single-query size; timing goes to
 * the "linear_query" profile bucket. */
int fhe_linear_queries_batch(fhe_ctx* ctx, const uint64_t* d_ct_q, int64_t Q, const void* d_docs8, int64_t B,
                             int32_t D, const int64_t* d_w, const int64_t* h_cst, uint64_t* d_out, void* stream);
/* fhe_compare_query_batch for Q seeded queries: d_qbody Q x D body words,
 * d_id0 Q stream ids (device), one public mask key, h_T Q thresholds (host).
 * Query q runs with cst - h_T[q]; d_acc[q B + b] is the accumulator and
 * d_below[q B + b] = 1 iff acc < h_T[q]. Single party: needs the secret key. */
int fhe_compare_queries_batch(fhe_ctx* ctx, const uint64_t* d_qbody, const uint64_t* d_id0,
                              const uint32_t h_mask_key[8], int64_t Q, const void* d_docs8, int64_t B, int32_t D,
                              const int64_t* d_w, int64_t cst, const int64_t* h_T, int64_t* d_acc, int64_t* d_below,
                              void* stream);
/* fhe_search_query_batch for Q seeded queries: result q B + b goes to
 * coefficient (q B + b) mod N of GLWE (q B + b) / N; d_glwe_acc (the values
 * acc - h_T[q]) and d_glwe_bit are ceil(Q B / N) x (k+1)N words each. Needs
 * evaluation keys and the packing key, no secret: works on a context made by
 * fhe_import_eval_keys. */
int fhe_search_queries_batch(fhe_ctx* ctx, const uint64_t* d_qbody, const uint64_t* d_id0,
                             const uint32_t h_mask_key[8], int64_t Q, const void* d_docs8, int64_t B, int32_t D,
                             const int64_t* d_w, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                             uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream);

/* ---- stored-ciphertext search: several queries in one pass -
 * Q CLEAR queries against the same B documents stored as seeded LWEs
 * (fhe_encrypt_seeded_batch: d_body B x D, d_id0 B stream ids, the public mask
 * key). Every mask block is regenerated once and meets the Q weight rows in
 * registers. Results are query-major (row / element q * B + b). Q >= 1,
 * B >= 1, D >= 1, Q <= 65535, B * D < 2^31, Q * B < 2^31, no null pointers:
 * otherwise FHE_E_ARG ("seeded queries ..." in fhe_last_error), reported before
 * the device and key checks; missing keys return FHE_E_STATE.
 *
 * The leveled step alone; needs no keys. d_W: Q x D (row-major, the caller has
 * folded 2^(P0-P) in), h_cst: Q host constants, d_out: Q*B x (kN+1):
 *   out[q B + b] = sum_j d_W[q][j] * ct(b, j) + trivial(h_cst[q] * Delta).
 * At Q = 1 word for word fhe_linear_seeded_batch. Timing goes to the
 * "linear_seeded" profile bucket. */
int fhe_linear_seeded_queries_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B, int32_t D,
                                    const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                    const int64_t* h_cst, uint64_t* d_out, void* stream);
/* fhe_compare_seeded_batch for Q weight rows: query q runs with cst - h_T[q];
 * d_acc[q B + b], d_below[q B + b] = [acc < h_T[q]]. Needs the secret key. */
int fhe_compare_seeded_queries_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                     int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                     int64_t cst, const int64_t* h_T, int64_t* d_acc, int64_t* d_below,
                                     void* stream);
/* evaluation-only: no decryption; result q B + b in coefficient (q B + b) mod N of GLWE (q B + b) / N,
 * ceil(Q B / N) GLWEs each for acc - h_T[q] (all levels) and the bits (levels_bit prefix; 0: all).
 * Needs evaluation keys and the packing key, no secret. */
int fhe_search_seeded_queries_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                    int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                    int64_t cst, const int64_t* h_T, int32_t levels_bit, uint64_t* d_glwe_acc,
                                    uint64_t* d_glwe_bit, void* stream);

/* ---- stored-ciphertext key rotation: bridge key switch ----
 * After a key rotation the stored seeded LWEs stay under the old big key. The
 * leveled step of the stored-ciphertext search is a clear-weight combination
 * of them, so its output is one big LWE per (query, document) under the OLD
 * key; one LWE -> LWE key switch with a bridge key (the old big key encrypted
 * under the new one) turns it into a ciphertext under the NEW key, and the
 * rest of the search runs with the new evaluation keys. No re-encryption, no
 * larger payloads; the host sees neither secret.
 *
 * Bridge key, gadget (base_log beta, level L; the packing gadget's bounds):
 * row (i, l), i < kN, l = 1..L, is an LWE under the new big key (dimension kN)
 * of the constant s_old[i] * 2^(64 - beta l), TUniform(glwe_noise_bits) noise,
 * ChaCha20 stream tags 33/34; layout [i][l][kN+1], fhe_bridge_key_words =
 * kN * L * (kN + 1) words (0 for a null params or a bad gadget). The bridge
 * of (a, b) is (0, .., 0, b) - sum_i sum_l d_{i,l} BK[i][l], d the balanced
 * digits of a_i (fhe_pack_batch's). It adds, in integer-word units,
 *   var_bridge = kN L ((B^2 + 2) / 12) tuniform_var(glwe_noise_bits)
 *                + (1 + kN / 2) 2^(2 (64 - beta L)) / 12,
 * fhe_pack_plan's model at count = 1; fhe_bridge_plan is fhe_pack_plan(params,
 * 1, in_var)'s gadget (host only; fheicp.params.bridge_plan is the same
 * function). Plan the packing key that follows with in_var + var_bridge / 2^128.
 *
 * Check order in every entry: argument errors (FHE_E_ARG: bad gadget, null
 * pointers, B_old outside [0, B], a key word other than 0 or 1) are reported
 * first, on host-only contexts too; then the device; then FHE_E_STATE ("no
 * bridge key", or a missing secret for the key generation). */
size_t fhe_bridge_key_words(const fhe_params* params, int32_t base_log, int32_t level);
int fhe_bridge_plan(const fhe_params* params, double in_var, int32_t* base_log, int32_t* level);
/* Generate the context's bridge key FROM the old big key h_s_big_old (kN host
 * words of 0/1, as fhe_export_keys writes s_big) TO the context's own secret
 * key (needed: FHE_E_STATE on an evaluation-only context). Replaces any
 * earlier bridge key. The device copy of the old key is zeroed and freed
 * before the call returns. */
int fhe_keygen_bridge_key_key(fhe_ctx* ctx, const uint64_t* h_s_big_old, int32_t base_log, int32_t level,
                              const uint32_t h_key[8], void* stream);
int fhe_keygen_bridge_key(fhe_ctx* ctx, const uint64_t* h_s_big_old, int32_t base_log, int32_t level, uint64_t seed,
                          void* stream);
/* Host copy of the bridge key / install one (converted once to byte planes
 * for the i8 matrix cores). Both work on an evaluation-only context. */
int fhe_export_bridge_key(fhe_ctx* ctx, uint64_t* h_out);
int fhe_import_bridge_key(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint64_t* h_in);
/* Bridge `count` contiguous big LWEs (kN+1 words each) from the old key to the
 * context's key; d_out may be d_ct. Needs only the bridge key. Bit-exact.
 * Timing goes to the "bridge" profile bucket. */
int fhe_bridge_batch(fhe_ctx* ctx, const uint64_t* d_ct, int64_t count, uint64_t* d_out, void* stream);
/* The same in place on the rows {q B + b : b < B_old} of a query-major Q x B
 * result (fhe_linear_seeded_queries_batch's d_out, the first B_old documents
 * under the old key): Q runs of B_old rows, not one block. Q >= 1, B >= 1,
 * 0 <= B_old <= B, Q * B < 2^31; every other row is left as it is, B_old = 0
 * does nothing. What fhe_search_seeded_queries_bridged_batch runs. */
int fhe_bridge_rows_batch(fhe_ctx* ctx, uint64_t* d_ct, int64_t Q, int64_t B, int64_t B_old, void* stream);
/* fhe_search_seeded_queries_batch with documents b < B_old (0 <= B_old <= B)
 * stored under the old key: the leveled step is unchanged, rows
 * {q B + b : b < B_old} of its result are bridged in place, then the sign
 * extraction and the two packings run as there. At B_old = 0 it is that entry
 * word for word and needs no bridge key. */
int fhe_search_seeded_queries_bridged_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                            int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                            int64_t cst, const int64_t* h_T, int32_t levels_bit, int64_t B_old,
                                            uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream);

/* ---- key rotation with several old generations resident ----
 * A rotation schedule leaves documents of several old generations resident.
 * The key holder makes one DIRECT bridge key from every still-resident old
 * generation to the current key (no chained bridges: a row carries the noise
 * of one bridge); the context holds them in FHE_BRIDGE_SLOTS bridge slots.
 * Slot 0 is the bridge key of the entries above, which keep working on it.
 * The *_slot entries are their siblings on the named slot: the same
 * arguments, outputs and check order, with "slot outside [0,
 * FHE_BRIDGE_SLOTS)" (FHE_E_ARG) first of all. The seeded keygen's "mask key
 * reuse" refusal covers every slot of the context (rows with equal masks under
 * one secret differ only by their messages, old key bits here); the unseeded
 * slot keygen refuses (FHE_E_ARG, "key reuse") a h_key another live slot of the
 * context was generated with, a courtesy and not the defence: draw every
 * slot's keys fresh. fhe_drop_bridge_key_slot frees a slot's words and planes
 * (an empty slot: nothing to do). */
#define FHE_BRIDGE_SLOTS 8
int fhe_keygen_bridge_key_slot_key(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                                   int32_t level, const uint32_t h_key[8], void* stream);
int fhe_keygen_bridge_key_slot(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                               int32_t level, uint64_t seed, void* stream);
int fhe_export_bridge_key_slot(fhe_ctx* ctx, int32_t slot, uint64_t* h_out);
int fhe_import_bridge_key_slot(fhe_ctx* ctx, int32_t slot, int32_t base_log, int32_t level, const uint64_t* h_in);
int fhe_drop_bridge_key_slot(fhe_ctx* ctx, int32_t slot);
/* Generation row map (G, h_ends, h_slots), host tables: documents are resident
 * oldest generation first and the current generation last; h_ends[G] is
 * non-decreasing with 0 <= h_ends[g] <= B, documents h_ends[g-1] <= b <
 * h_ends[g] (h_ends[-1] = 0) belong to old generation g and bridge slot
 * h_slots[g] bridges them; documents b >= h_ends[G-1] are under the current
 * key. Empty generations are allowed. fhe_bridge_gens_batch works in place on
 * a query-major Q x B result (Q >= 1, B >= 1, Q * B < 2^31); every row of a
 * current-key document is left untouched. One digits launch, one GEMM on the
 * i8 matrix cores with each 128-row block's own key planes, and one copy back
 * serve all generations (a -DFHEICP_GRP_BRIDGE=0 build runs one single-key
 * bridge per generation behind the same entries); bit-exact, equal word for
 * word to the single bridge applied generation by generation. Timing goes to
 * the "bridge" bucket.
 * FHE_E_ARG first, on host-only contexts too: G outside [0,
 * FHE_BRIDGE_SLOTS], null tables when G > 0, ends that decrease or exceed B, a
 * slot out of range or named twice. Then the device. Then FHE_E_STATE: a
 * named slot with rows but no key ("no bridge key in slot s"), named slots
 * with rows whose gadgets differ ("bridge gadgets differ"). More than 65,535
 * digit groups of 16 rows or 8,191 blocks of 128 rows over all generations is
 * FHE_E_ARG ("split the call"), before anything is queued. */
int fhe_bridge_gens_batch(fhe_ctx* ctx, uint64_t* d_ct, int64_t Q, int64_t B, int32_t G, const int64_t* h_ends,
                          const int32_t* h_slots, void* stream);
/* fhe_search_seeded_queries_bridged_batch with the generation row map in
 * B_old's place. At G = 0 it is fhe_search_seeded_queries_batch word for word
 * and needs no bridge key; at G = 1, h_slots = {0} it is the bridged entry
 * word for word. */
int fhe_search_seeded_queries_gens_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t B,
                                         int32_t D, const uint32_t h_mask_key[8], int64_t Q, const int64_t* d_W,
                                         int64_t cst, const int64_t* h_T, int32_t levels_bit, int32_t G,
                                         const int64_t* h_ends, const int32_t* h_slots, uint64_t* d_glwe_acc,
                                         uint64_t* d_glwe_bit, void* stream);

/* ---- both-private search: several GGSW queries in one pass -
 * Q GGSW queries of one key holder (d_ggsw: Q x fhe_ggsw_words, one gadget)
 * against the same B GLWE-encrypted documents. The product is the one of
 * fhe_linear_ggsw_batch, transposed: rows (q, component), K = (c, l, coef),
 * columns (document GLWE, coef); the query operand is the GGSWs' own byte
 * planes and the document fragments are formed in the kernel, so no buffer
 * is proportional to ((k+1)N)^2 and the Q queries share every document
 * fragment. Results are query-major (row / element q * B + b) and equal, word
 * for word, Q single-query calls. Q >= 1, B >= 1, 0 < D <= N, Q <= 65535,
 * Q * B < 2^31, the gadget bounds of fhe_encrypt_ggsw, N a multiple of 256,
 * no null pointers: otherwise FHE_E_ARG ("ggsw queries ..." in
 * fhe_last_error), reported before the device and key checks; missing keys
 * return FHE_E_STATE.
 *
 * The resident document operand of the batched entries, once per corpus:
 * 2N + 16 bytes per (document GLWE, component, level), the digits of
 * fhe_glwe_docs_pack (same rounding, same tie coins) reversed and followed by
 * their negation. fhe_glwe_docs_queries_bytes is 0 for bad arguments. */
size_t fhe_glwe_docs_queries_bytes(const fhe_params* params, int64_t B, int32_t D, int32_t level);
int fhe_glwe_docs_queries_pack(fhe_ctx* ctx, const uint64_t* d_glwe, int64_t B, int32_t D, int32_t base_log,
                               int32_t level, void* d_docs, void* stream);
/* Bytes of context-owned workspace a batched call allocates on first use
 * (byte planes of the padded rows | the Q x G x (k+1)N result | Q constants);
 * the Q * B results' own workspace is the other batched entries'. Host only;
 * 0 for bad arguments. */
size_t fhe_ggsws_ws_bytes(const fhe_params* params, int64_t Q, int64_t B, int32_t D, int32_t level);
/* The leveled step alone; needs no keys. h_cst: Q host constants; d_out:
 * Q*B x (kN+1), row q B + b = document b under query q with
 * trivial(h_cst[q] Delta) added. Timing goes to the "linear_ggsws" profile
 * bucket (planes + GEMM + slot extraction, one bracket). */
int fhe_linear_ggsws_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs,
                           int64_t Q, int64_t B, int32_t D, const int64_t* h_cst, uint64_t* d_out, void* stream);
/* fhe_compare_ggsw_batch for Q queries: query q runs with cst - h_T[q];
 * d_acc[q B + b], d_below[q B + b] = [acc < h_T[q]]. Needs the secret key. */
int fhe_compare_ggsws_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs,
                            int64_t Q, int64_t B, int32_t D, int64_t cst, const int64_t* h_T, int64_t* d_acc,
                            int64_t* d_below, void* stream);
/* evaluation-only: result q B + b in coefficient (q B + b) mod N of GLWE (q B + b) / N, ceil(Q B / N) GLWEs
 * each for acc - h_T[q] (all levels) and the bits (levels_bit prefix; 0: all). Needs evaluation keys and the
 * packing key, no secret. */
int fhe_search_ggsws_batch(fhe_ctx* ctx, const uint64_t* d_ggsw, int32_t base_log, int32_t level, const void* d_docs,
                           int64_t Q, int64_t B, int32_t D, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                           uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream);

/* ---- several key holders in one batched call -------------
 * A group borrows T contexts (1 <= T <= 64, no null, no repeat), all on one
 * device and with equal fhe_params (msg_bits included: re-checked at every
 * call), whose sign schedule runs only rotations that have a group form: the
 * multi-bit ones at N = 1024, k = 2 and the generic one (every planned set
 * from P = 4 to 26 and the toy set; a set with a classic round at N = 1024 is
 * refused, "group: round r runs the classic rotation"). Checks in that order
 * (FHE_E_ARG, "group" in fhe_last_error(NULL); host-only contexts report them
 * too), then evaluation keys on every context (FHE_E_STATE). The contexts
 * must outlive the group; a group is used from one thread at a time, and its
 * calls use the contexts' key-switch and packing workspaces.
 *
 * Row layout of a group batch: T segments, tenant t with counts[t] >= 0 rows
 * at start_t = sum_{u<t} 4 ceil(counts[u] / 4); fhe_group_rows returns the
 * padded total M and writes the T starts (host only; -1 for null or negative
 * counts). Rows start_t + counts[t] .. start_{t+1} - 1 are padding, neither
 * read nor written. */
typedef struct fhe_group fhe_group;
int fhe_group_create(fhe_ctx* const* ctxs, int32_t T, fhe_group** out);
void fhe_group_destroy(fhe_group* group);
int64_t fhe_group_rows(const int64_t* counts, int32_t T, int64_t* starts);
/* fhe_sign_batch over the padded layout (d_ct_v, d_sign: M x (kN+1), d_ct_v
 * consumed): the same schedule, shifts and test vectors; per round tenant t's
 * rows take t's key switch, then one rotation launch serves every tenant,
 * each workgroup with its own tenant's key. On the caller's stream, no
 * two-half pipelining. sum counts < 2^31; all zero returns FHE_OK. */
int fhe_sign_group_batch(fhe_group* group, uint64_t* d_ct_v, const int64_t* h_counts, uint64_t* d_sign, void* stream);
/* One tenant's part of fhe_search_query_group_batch: the arguments of
 * fhe_search_queries_batch. Q = 0: the tenant sits this call out. */
typedef struct fhe_group_query {
  int32_t struct_size;        /* = sizeof(fhe_group_query); else FHE_E_ARG */
  int32_t D;
  const uint64_t* d_qbody;    /* Q x D body words */
  const uint64_t* d_id0;      /* Q stream ids (device) */
  const uint32_t* h_mask_key; /* 8 words */
  int64_t Q;
  const void* d_docs8;        /* fhe_query_docs_pack of the tenant's B documents */
  int64_t B;
  const int64_t* d_w;
  int64_t cst;
  const int64_t* h_T;         /* Q thresholds (host) */
  int32_t levels_bit;
  int32_t reserved;           /* 0 */
  uint64_t* d_glwe_acc;       /* ceil(Q B / N) x (k+1)N words */
  uint64_t* d_glwe_bit;
} fhe_group_query;
/* The evaluation-only server of fhe_search_queries_batch for the T tenants of
 * a group (items[t] for context t): per tenant the expansion and leveled GEMM
 * into its segment, one fhe_sign_group_batch over all segments, then the
 * tenant's two packings with its own packing key. Tenant t's outputs are word
 * for word those of fhe_search_queries_batch on its own context (result order
 * q * B + b). Argument errors (FHE_E_ARG) come before the device and key
 * checks; a participating tenant without a packing key is FHE_E_STATE. */
int fhe_search_query_group_batch(fhe_group* group, const fhe_group_query* items, int32_t T, void* stream);

/* ---- a group's key switch and stored-ciphertext search ---
 * Host only: 1 when every round of the parameter set's sign schedule has a
 * group kernel (fhe_group_create accepts contexts of it), 0 when a round runs
 * the classic rotation, FHE_E_ARG for an invalid set. */
int fhe_group_form(const fhe_params* params);
/*
 * fhe_keyswitch_batch over the padded layout (d_big: M x (kN+1), d_small:
 * M x (n+1)): tenant t's rows with tenant t's key, word for word its own
 * fhe_keyswitch_batch; padding rows are neither read nor written. With every
 * tenant on the MFMA variant it is one digits launch and one GEMM launch
 * whose 128-ciphertext workgroups each take their tenant's key planes from a
 * table (timing: tenant 0's "keyswitch" bucket, k_keyswitch_mfma_grp<...>);
 * otherwise one key switch per tenant. Checks as fhe_sign_group_batch, in its
 * order, with fhe_keyswitch_batch's shift bound among the argument checks.
 * More than 65535 digit groups (16 rows each, rounded up per tenant) or 8191
 * blocks (128 rows each, rounded up per tenant) over ALL tenants of one call:
 * FHE_E_ARG, "split the call", before any work is queued; the same bound
 * holds for fhe_sign_group_batch and the two group search entries when they
 * run the grouped key switch. */
int fhe_keyswitch_group_batch(fhe_group* group, const uint64_t* d_big, const int64_t* h_counts, int32_t shift,
                              uint64_t add_body, uint64_t* d_small, void* stream);
/* One tenant's part of fhe_search_seeded_queries_group_batch: the arguments
 * of fhe_search_seeded_queries_bridged_batch. Q = 0: the tenant sits this
 * call out. */
typedef struct fhe_group_corpus {
  int32_t struct_size;        /* = sizeof(fhe_group_corpus); else FHE_E_ARG */
  int32_t D;
  const uint64_t* d_body;     /* B x D body words of the stored documents */
  const uint64_t* d_id0;      /* B stream ids (device) */
  int64_t B;
  const uint32_t* h_mask_key; /* 8 words */
  int64_t Q;
  const int64_t* d_W;         /* Q x D weight rows */
  int64_t cst;
  const int64_t* h_T;         /* Q thresholds (host) */
  int32_t levels_bit;
  int32_t reserved;           /* 0 */
  int64_t B_old;              /* documents b < B_old are under the rotated-out key */
  uint64_t* d_glwe_acc;       /* ceil(Q B / N) x (k+1)N words */
  uint64_t* d_glwe_bit;
} fhe_group_corpus;
/* The evaluation-only server of fhe_search_seeded_queries_bridged_batch for
 * the T tenants of a group (items[t] for context t): per tenant the leveled
 * step into its segment and, where B_old > 0, the bridge on its old
 * documents' rows with its own bridge key; one fhe_sign_group_batch over all
 * segments; then the tenant's two packings with its own packing key. Tenant
 * t's outputs are word for word those of that entry on its own context.
 * FHE_E_ARG first ("tenant t: ...": struct_size, the entry's bounds, nulls,
 * B_old outside [0, B], levels_bit, 2^31 results and more), then the device,
 * then FHE_E_STATE (no packing key, or no bridge key where B_old > 0). */
int fhe_search_seeded_queries_group_batch(fhe_group* group, const fhe_group_corpus* items, int32_t T, void* stream);

/* ---- rotation schedules in a group: one bridge for all tenants -
 * One tenant's part of a group bridge: its query-major Q x B result and its
 * generation row map (G, h_ends, h_slots) as fhe_bridge_gens_batch takes it. */
typedef struct fhe_group_rowmap {
  int32_t struct_size;        /* = sizeof(fhe_group_rowmap); else FHE_E_ARG */
  int32_t G;                  /* G old generations, 0..FHE_BRIDGE_SLOTS */
  int64_t Q;                  /* Q = 0: the tenant sits this call out */
  int64_t B;
  const int64_t* h_ends;      /* G, as fhe_bridge_gens_batch */
  const int32_t* h_slots;     /* G */
} fhe_group_rowmap;
/* fhe_bridge_gens_batch for the T tenants of a group, in place on the padded
 * layout of counts[t] = Q_t * B_t (fhe_group_rows): tenant t's segment is, word
 * for word, what fhe_bridge_gens_batch on t's own context gives; padding rows,
 * current-key rows and the rows of tenants that sit out are neither read nor
 * written. Every non-empty old generation of every participating tenant is one
 * segment of ONE pass: the tables, one digits launch, one GEMM on the i8 matrix
 * cores whose 128-row blocks each take their segment's key planes, one copy
 * back. Tenants whose bridge gadgets differ run one pass per distinct
 * (base_log, level), in order of first appearance. Timing goes to the "bridge"
 * bucket of the group's first context, one bracket per pass.
 * FHE_E_ARG first ("tenant t: ...", before the device is looked at):
 * struct_size, Q < 0, Q * B >= 2^31, fhe_bridge_gens_batch's row-map rules, a
 * null d_ct, 2^31 results and more. Then the device and the evaluation keys.
 * Then FHE_E_STATE: "tenant t: no bridge key in slot s" for a named slot with
 * rows, "tenant t: bridge gadgets differ" within one tenant. More than 65,535
 * digit groups of 16 rows or 8,191 blocks of 128 rows over all segments of a
 * pass is FHE_E_ARG ("split the call"), before anything is queued. */
int fhe_bridge_group_gens_batch(fhe_group* group, uint64_t* d_ct, const fhe_group_rowmap* maps, int32_t T,
                                void* stream);
/* One tenant's part of fhe_search_seeded_queries_group_gens_batch:
 * fhe_group_corpus with the generation row map in B_old's place. Q = 0: the
 * tenant sits this call out. */
typedef struct fhe_group_corpus_gens {
  int32_t struct_size;        /* = sizeof(fhe_group_corpus_gens); else FHE_E_ARG */
  int32_t D;
  const uint64_t* d_body;     /* B x D body words of the stored documents */
  const uint64_t* d_id0;      /* B stream ids (device) */
  int64_t B;
  const uint32_t* h_mask_key; /* 8 words */
  int64_t Q;
  const int64_t* d_W;         /* Q x D weight rows */
  int64_t cst;
  const int64_t* h_T;         /* Q thresholds (host) */
  int32_t levels_bit;
  int32_t G;                  /* old generations, 0..FHE_BRIDGE_SLOTS */
  const int64_t* h_ends;      /* G: documents h_ends[g-1] <= b < h_ends[g] are under old generation g */
  const int32_t* h_slots;     /* G: the bridge slot of each */
  uint64_t* d_glwe_acc;       /* ceil(Q B / N) x (k+1)N words */
  uint64_t* d_glwe_bit;
} fhe_group_corpus_gens;
/* fhe_search_seeded_queries_group_batch with every tenant's rotation schedule:
 * the leveled steps, the group bridge above over all tenants' old generations,
 * one fhe_sign_group_batch, the packings. Tenant t's outputs are word for word
 * those of fhe_search_seeded_queries_gens_batch on its own context; with every
 * tenant at G <= 1 and slot 0 they are those of
 * fhe_search_seeded_queries_group_batch. Checks: that entry's, with the row-map
 * rules in B_old's place, then the group bridge's FHE_E_STATE checks after the
 * packing key's, then its launch limit. */
int fhe_search_seeded_queries_group_gens_batch(fhe_group* group, const fhe_group_corpus_gens* items, int32_t T,
                                               void* stream);

/* ---- both-private search for a group ---------------------
 * One tenant's part of the two entries below: the arguments of
 * fhe_search_ggsws_batch. Q = 0: the tenant sits this call out. */
typedef struct fhe_group_ggsw {
  int32_t struct_size;        /* = sizeof(fhe_group_ggsw); else FHE_E_ARG */
  int32_t D;
  const uint64_t* d_ggsw;     /* Q GGSW queries of gadget (base_log, level) */
  int32_t base_log;
  int32_t level;              /* one level for all participating tenants of a call */
  const void* d_docs;         /* fhe_glwe_docs_queries_pack of the tenant's B documents */
  int64_t Q;
  int64_t B;
  int64_t cst;
  const int64_t* h_T;         /* Q thresholds (host); the search entry only */
  int32_t levels_bit;
  int32_t reserved;           /* 0 */
  uint64_t* d_glwe_acc;       /* ceil(Q B / N) x (k+1)N words; the search entry only */
  uint64_t* d_glwe_bit;
} fhe_group_ggsw;
/* The leveled step of fhe_linear_ggsws_batch for the T tenants of a group in
 * a number of launches that does not depend on T: one tables step, one plane
 * launch, one grouped transposed external product (k_extprod_queries_mfma_grp,
 * tenant t's queries against tenant t's documents), one slot extraction, and
 * one memset when K is split. d_out: the padded layout M x (kN+1) of
 * fhe_group_rows with counts[t] = Q_t B_t; tenant t's rows (query-major, with
 * trivial(h_cst[t][q] Delta) added) are word for word those of
 * fhe_linear_ggsws_batch on its own context, and padding rows are neither read
 * nor written. Needs a group but uses no key. cst, h_T, levels_bit and the two
 * outputs of the items are ignored. Timing goes to tenant 0's "linear_ggsws"
 * bucket (one bracket). FHE_E_ARG first ("tenant t: ...": struct_size,
 * reserved, fhe_linear_ggsws_batch's bounds, nulls, a level that differs from
 * the first participating tenant's, 2^31 results and more; a launch beyond
 * 2^31 tiles: "split the call"), then the device. */
int fhe_linear_ggsws_group_batch(fhe_group* group, const fhe_group_ggsw* items, int32_t T,
                                 const int64_t* const* h_cst, uint64_t* d_out, void* stream);
/* The evaluation-only server of fhe_search_ggsws_batch for the T tenants of a
 * group (items[t] for context t): the grouped leveled step above with
 * cst - h_T[q] on query q (it also writes the copy the packings read), one
 * fhe_sign_group_batch over all segments, then the tenant's two packings with
 * its own packing key. Tenant t's outputs are word for word those of
 * fhe_search_ggsws_batch on its own context. FHE_E_ARG first (as above, and
 * levels_bit), then the device, then FHE_E_STATE (no packing key). All tenants
 * with Q = 0 returns FHE_OK. */
int fhe_search_ggsws_group_batch(fhe_group* group, const fhe_group_ggsw* items, int32_t T, void* stream);

/* ---- both-private search: seeded documents and queries ----
 * In a document GLWE and in every GGSW row, k of the k+1 polynomials are
 * uniform masks. The seeded forms keep the body polynomial alone: the masks
 * are words of ChaCha20 streams under a PUBLIC mask key that travels with the
 * payload, the noise comes from a SECRET noise key that never leaves the
 * client. Tags, stream ids and word addressing are the full forms':
 *   document GLWE g, component i < k:  word iN + t of (tag 7, id0 + g),
 *   GGSW row r = cL + l, component c': word t of (tag 31, id0 + r k + c'),
 * so with mask key = noise key = K the expansion of a seeded ciphertext is,
 * word for word, the full-form ciphertext under K (tests only: a deployment
 * never sets the two equal). An id must not repeat under one mask key.
 * A seeded document GLWE is N words instead of (k+1)N, a seeded GGSW
 * fhe_ggsw_body_words = (k+1) L N instead of fhe_ggsw_words (0 for a null
 * params or a bad gadget).
 *
 * Argument errors (null pointers or keys, D > N, a bad gadget, Q or B outside
 * the full-form sibling's range) return FHE_E_ARG with "seeded" in
 * fhe_last_error and come first, on host-only contexts too; then the device
 * (FHE_E_DEVICE), then missing keys (FHE_E_STATE). */
size_t fhe_ggsw_body_words(const fhe_params* params, int32_t base_log, int32_t level);
/* fhe_encrypt_packed_batch_key / fhe_encrypt_ggsw_key with the key split in
 * two and the bodies alone as output: d_body B x ceil(D / N) x N words, and
 * (k+1) L x N words [c][l][coef]. Both need the secret key. */
int fhe_encrypt_packed_seeded_batch(fhe_ctx* ctx, const int64_t* d_qx, int64_t B, int32_t D,
                                    const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], uint64_t id0,
                                    uint64_t* d_body, void* stream);
int fhe_encrypt_ggsw_seeded(fhe_ctx* ctx, const int64_t* d_w, int32_t D, int32_t base_log, int32_t level,
                            const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], uint64_t id0,
                            uint64_t* d_body, void* stream);
/* Bodies -> full form (k_expand_ggsw_seeded); no keys needed. Documents:
 * B x ceil(D / N) GLWEs of (k+1)N words, GLWE g under stream id id0 + g.
 * Queries: d_body Q x fhe_ggsw_body_words, d_id0 Q stream ids (device),
 * d_ggsw Q x fhe_ggsw_words; 1 <= Q <= 65535. Timing goes to the
 * "expand_ggsw_seeded" profile bucket. */
int fhe_expand_packed_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int64_t B, int32_t D,
                                   const uint32_t h_mask_key[8], uint64_t* d_glwe, void* stream);
int fhe_expand_ggsws_seeded(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int64_t Q, int32_t base_log,
                            int32_t level, const uint32_t h_mask_key[8], uint64_t* d_ggsw, void* stream);
/* fhe_glwe_docs_pack / fhe_glwe_docs_queries_pack from seeded documents:
 * d_body ceil(B / (N / D)) x N body words, document GLWE g under stream id
 * id0 + g. The operands (fhe_glwe_docs_bytes, fhe_glwe_docs_queries_bytes) are
 * byte for byte those of the full-form entries on the expanded GLWEs; the
 * masks are regenerated in registers, no full-form GLWE exists on host or
 * device. (k+1)N a multiple of 128. No keys needed. */
int fhe_glwe_docs_pack_seeded(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int64_t B, int32_t D,
                              int32_t base_log, int32_t level, const uint32_t h_mask_key[8], void* d_docs8,
                              void* stream);
int fhe_glwe_docs_queries_pack_seeded(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int64_t B, int32_t D,
                                      int32_t base_log, int32_t level, const uint32_t h_mask_key[8], void* d_docs,
                                      void* stream);
/* fhe_search_ggsw_batch / fhe_search_ggsws_batch on seeded queries: the
 * queries are expanded into a context-owned workspace (Q x fhe_ggsw_words,
 * allocated on first use), then the full-form entry runs unchanged; the
 * outputs are those of the full-form entry on the expanded queries. */
int fhe_search_ggsw_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, uint64_t id0, int32_t base_log, int32_t level,
                                 const uint32_t h_mask_key[8], const void* d_docs8, int64_t B, int32_t D, int64_t cst,
                                 int64_t T, int32_t levels_bit, uint64_t* d_glwe_acc, uint64_t* d_glwe_bit,
                                 void* stream);
int fhe_search_ggsws_seeded_batch(fhe_ctx* ctx, const uint64_t* d_body, const uint64_t* d_id0, int32_t base_log,
                                  int32_t level, const uint32_t h_mask_key[8], const void* d_docs, int64_t Q,
                                  int64_t B, int32_t D, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                                  uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream);

/* ---- seeded evaluation keys ------------------------------
 * Every row of an evaluation key is uniform mask words from a ChaCha20 stream
 * and a body. The seeded form of a key is the body of every row and the PUBLIC
 * mask key the masks came from; the secrets and every noise word come from a
 * SECRET noise key that never leaves the client. Tags, stream ids and word
 * addressing are those of fhe_keygen_key:
 *   GLWE rows (bsk, the gadgets' keys, the packing key): row r, component
 *     c < k, is words [0, N) of (mask tag, r k + c); the body is the last N of
 *     the row's (k+1)N words;
 *   LWE rows (ksk, the bridge key): row r is words [0, n1 - 1) of (mask tag, r);
 *     the body is the last of the row's n1 words (n1 = n + 1, kN + 1).
 * Every mask word of a seeded key is a stream word. fhe_keygen_key's
 * bootstrapping keys are NOT of that form: a GGSW row (i, c, l) with c < k
 * carries its message s_i g_l in word cN of the MASK, and a mask word that
 * differs from a public stream by s_i g_l would give s_i away. The seeded
 * keygen writes the same encryption with the message in the body: mask =
 * stream, body = fhe_keygen_key's body - s_i g_l S_c (the phase is e - s_i g_l
 * S_c in both). So with mask key = noise key = K the set is fhe_keygen_key(K)'s
 * word for word in ksk, packing and bridge key and in every bsk row but those
 * (c < k, s_i = 1), which differ by exactly that move: same secrets, same
 * noise, same phases (tests only: a deployment never sets the two equal).
 * fhe_keygen_key's words are unchanged. ONE MASK KEY SERVES ONE
 * GENERATED KEY: the main set (bsk, gadget keys, ksk: distinct tags) shares
 * one, the packing key has its own and so has the bridge key; rows with equal
 * masks under one secret differ by messages and noise alone.
 *
 * Body sizes in words (0 for a null params, a bad gadget or an absent fast
 * gadget, as the full-form siblings): n (k+1) L N, kN ks_level, a (k+1)-th of
 * fhe_fast_bsk_words, kN L N and kN L. */
size_t fhe_bsk_body_words(const fhe_params* params);
size_t fhe_ksk_body_words(const fhe_params* params);
size_t fhe_fast_bsk_body_words(const fhe_params* params, int32_t which);
size_t fhe_pack_key_body_words(const fhe_params* params, int32_t base_log, int32_t level);
size_t fhe_bridge_key_body_words(const fhe_params* params, int32_t base_log, int32_t level);
/* fhe_keygen_key, fhe_keygen_pack_key_key and fhe_keygen_bridge_key_key with
 * the key split in two; the secrets are the noise key's. The context remembers
 * each key's mask key. A packing or bridge keygen whose mask key a seeded
 * keygen of this context already used returns FHE_E_ARG ("mask key reuse": a
 * courtesy, not the defence). Argument errors say "seeded" and come before the
 * device and key checks. */
int fhe_keygen_seeded(fhe_ctx* ctx, const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], void* stream);
int fhe_keygen_pack_key_seeded(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_mask_key[8],
                               const uint32_t h_noise_key[8], void* stream);
int fhe_keygen_bridge_key_seeded(fhe_ctx* ctx, const uint64_t* h_s_big_old, int32_t base_log, int32_t level,
                                 const uint32_t h_mask_key[8], const uint32_t h_noise_key[8], void* stream);
/* The mask key and the bodies (host buffers of the sizes above;
 * h_gadget_body[g - 1] for every gadget the parameters have). FHE_E_STATE
 * naming "seeded" when the key was not generated or imported with a mask key:
 * after fhe_keygen_key, a full-form import, and for the fast gadgets' keys
 * after fhe_import_keys (re-encrypted under a private random key). */
int fhe_export_eval_keys_seeded(fhe_ctx* ctx, uint32_t h_mask_key_out[8], uint64_t* h_bsk_body, uint64_t* h_ksk_body,
                                uint64_t* const h_gadget_body[5]);
int fhe_export_pack_key_seeded(fhe_ctx* ctx, uint32_t h_mask_key_out[8], uint64_t* h_body);
int fhe_export_bridge_key_seeded(fhe_ctx* ctx, uint32_t h_mask_key_out[8], uint64_t* h_body);
/* Evaluation-only import: the bodies are copied to a staging buffer, the keys
 * expanded into the context's standard-form buffers (k_expand_ggsw_seeded,
 * k_expand_lwe_rows_seeded) and converted as by the full-form imports, whose
 * result this equals. fhe_import_eval_keys_seeded behaves as
 * fhe_import_eval_keys: no secret is allocated, secrets already present are
 * zeroed and freed. The context keeps the mask key, so it can export the keys
 * seeded again. */
int fhe_import_eval_keys_seeded(fhe_ctx* ctx, const uint32_t h_mask_key[8], const uint64_t* h_bsk_body,
                                const uint64_t* h_ksk_body, const uint64_t* const h_gadget_body[5]);
int fhe_import_pack_key_seeded(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_mask_key[8],
                               const uint64_t* h_body);
int fhe_import_bridge_key_seeded(fhe_ctx* ctx, int32_t base_log, int32_t level, const uint32_t h_mask_key[8],
                                 const uint64_t* h_body);
/* The seeded bridge entries on a named bridge slot: "slot
 * outside [0, FHE_BRIDGE_SLOTS)" first, then their siblings' checks. */
int fhe_keygen_bridge_key_slot_seeded(fhe_ctx* ctx, int32_t slot, const uint64_t* h_s_big_old, int32_t base_log,
                                      int32_t level, const uint32_t h_mask_key[8], const uint32_t h_noise_key[8],
                                      void* stream);
int fhe_export_bridge_key_slot_seeded(fhe_ctx* ctx, int32_t slot, uint32_t h_mask_key_out[8], uint64_t* h_body);
int fhe_import_bridge_key_slot_seeded(fhe_ctx* ctx, int32_t slot, int32_t base_log, int32_t level,
                                      const uint32_t h_mask_key[8], const uint64_t* h_body);

/* ---- both-private key rotation: per-generation GGSW queries
 * After a key rotation the documents of several generations are resident,
 * each generation's GLWEs under its own big key. The client sends every query
 * once per resident generation, as a GGSW under THAT generation's key; the
 * host multiplies generation g's documents by generation g's GGSWs (the exact
 * product of fhe_linear_ggsws_batch, nothing switched before it), extracts big
 * LWEs under the old keys and moves those rows to the current key with the
 * grouped bridge of fhe_bridge_gens_batch. The bridge's noise is added to the
 * product's, not multiplied by the query's norm.
 *
 * One generation's part of a call. Generations come oldest first,
 * 1 <= G <= FHE_BRIDGE_SLOTS + 1; at most one entry has slot -1 and it is the
 * last; no slot is named twice; B = sum B_g >= 1. Document b of generation g
 * is document off_g + b of the call, off_g = sum_{h<g} B_h (a generation's
 * documents start a new GLWE of its own operand). */
typedef struct fhe_ggsw_gen {
  int32_t struct_size;     /* = sizeof(fhe_ggsw_gen); else FHE_E_ARG */
  int32_t slot;            /* bridge slot of this generation's key; -1: the context's current key */
  const uint64_t* d_ggsw;  /* Q GGSWs under THIS generation's big key, gadget (base_log, level) */
  const void* d_docs;      /* fhe_glwe_docs_queries_pack of this generation's B documents */
  int64_t B;               /* 0: an empty generation, pointers ignored */
} fhe_ggsw_gen;
/* Bytes of product workspace a call takes for its byte planes, results and
 * constants: fhe_ggsws_ws_bytes summed over the generations with documents,
 * the Q constants counted once (G = 1: fhe_ggsws_ws_bytes itself). The
 * launch's tables (56 bytes per generation, 16 per workgroup tile, 4 per row
 * tile) follow them and are not counted. Host only; 0 for bad arguments. */
size_t fhe_ggsws_gens_ws_bytes(const fhe_params* params, int64_t Q, const int64_t* h_B, int32_t G, int32_t D,
                               int32_t level);
/* The leveled step alone; needs no key and bridges nothing. d_out:
 * Q*B x (kN+1); row q B + off_g + b is generation g's document b under
 * generation g's query q with trivial(h_cst[q] Delta) added, under generation
 * g's key: word for word row q B_g + b of fhe_linear_ggsws_batch on that
 * generation's operands. The launch count does not depend on G (one tables
 * kernel, one plane launch, one grouped transposed product, one extraction,
 * one memset when K is split). Timing goes to the "linear_ggsws" bucket.
 * FHE_E_ARG first, on host-only contexts too (struct_size, G, slots, nulls,
 * fhe_linear_ggsws_batch's bounds, a launch beyond 2^31 tiles: "split the
 * call"), then the device. */
int fhe_linear_ggsws_gens_batch(fhe_ctx* ctx, const fhe_ggsw_gen* gens, int32_t G, int32_t base_log, int32_t level,
                                int64_t Q, int32_t D, const int64_t* h_cst, uint64_t* d_out, void* stream);
/* The evaluation-only server: the leveled step with cst - h_T[q], the grouped
 * bridge over the rows of the generations with slot >= 0 (timing: "bridge"),
 * the sign extraction and the two packings of fhe_search_ggsws_batch, the
 * packings' copy taken after the bridge. Outputs as fhe_search_ggsws_batch
 * with B = sum B_g. G = 1 with slot -1 equals fhe_search_ggsws_batch word for
 * word; old generations only (no slot -1 entry) is allowed. FHE_E_ARG first
 * (as above, and levels_bit), then the device, then FHE_E_STATE: no keys, no
 * packing key, "no bridge key in slot s" for a named slot with rows, "bridge
 * gadgets differ". */
int fhe_search_ggsws_gens_batch(fhe_ctx* ctx, const fhe_ggsw_gen* gens, int32_t G, int32_t base_log, int32_t level,
                                int64_t Q, int32_t D, int64_t cst, const int64_t* h_T, int32_t levels_bit,
                                uint64_t* d_glwe_acc, uint64_t* d_glwe_bit, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* FHE_ICP_H */
