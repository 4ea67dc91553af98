"""Reference-side ctypes binding of libfheicp.so (no torch, numpy only).

This is the file a maintainer of the reference would add next to
fhe_similarity.py to call the MI355X engine through its C ABI
(include/fhe_icp.h) directly; INTEGRATION.md shows where it plugs in. It is
kept here, runnable, so tests/test_gpu_dropin.py can prove that the binding
works as written.

    eng = GpuCompare(params_dict, lib_path=".../libfheicp.so")
    acc, below = eng.compare(q_x, q_w, cst, T)   # int64 numpy arrays

Keys come from 32 bytes of os.urandom (fhe_keygen_key) and every session
encrypts under its own 32-byte stream key with a random 64-bit id start
(fhe_compare_batch_key / fhe_score_batch_key). key_seed / enc_seed select the
64-bit seed forms, for reproducible tests only.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

FIELDS = ("n", "k", "N", "pbs_base_log", "pbs_level", "ks_base_log", "ks_level",
          "lwe_noise_bits", "glwe_noise_bits", "msg_bits", "sign_digit_bits",
          "pbs_fast_base_log", "pbs_fast_level", "pbs_fast2_base_log", "pbs_fast2_level",
          "pbs_fast_group", "pbs_fast2_group", "pbs_mid_base_log", "pbs_mid_level", "pbs_mid2_base_log",
          "pbs_mid2_level", "pbs_mid_group", "pbs_mid2_group", "pbs_mid0_base_log", "pbs_mid0_level",
          "pbs_mid0_group")


class fhe_params(C.Structure):
    # struct_size (= sizeof(fhe_params), checked by the library) leads
    _fields_ = [("struct_size", C.c_int32)] + [(f, C.c_int32) for f in FIELDS]


class fhe_ggsw_gen(C.Structure):
    # one key generation's part of the *_ggsws_gens_batch entries: slot -1 is the current key
    _fields_ = [("struct_size", C.c_int32), ("slot", C.c_int32), ("d_ggsw", C.c_void_p), ("d_docs", C.c_void_p),
                ("B", C.c_int64)]


_vp, _i32, _i64, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
_PROTOS = {
    "fhe_ctx_create": (C.c_int, [C.POINTER(fhe_params), C.c_int, C.POINTER(_vp)]),
    "fhe_ctx_destroy": (None, [_vp]),
    "fhe_last_error": (C.c_char_p, [_vp]),
    "fhe_keygen": (C.c_int, [_vp, _u64, _vp]),
    "fhe_keygen_key": (C.c_int, [_vp, _vp, _vp]),
    "fhe_dev_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "fhe_dev_free": (C.c_int, [_vp, _vp]),
    "fhe_memcpy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "fhe_memcpy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "fhe_compare_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _i64, _u64, _u64, _vp, _vp, _vp]),
    "fhe_topk": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "fhe_score_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _i64, _u64, _u64, _vp, _vp]),
    "fhe_compare_batch_key": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _i64, _vp, _u64, _vp, _vp, _vp]),
    "fhe_score_batch_key": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _i64, _vp, _u64, _vp, _vp]),
    # private query over a plaintext store
    "fhe_set_msg_bits": (C.c_int, [_vp, _i32]),
    "fhe_encrypt_seeded_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fhe_query_docs_bytes": (C.c_size_t, [C.POINTER(fhe_params), _i64, _i32]),
    "fhe_query_docs_pack": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "fhe_linear_query_batch": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    "fhe_compare_query_batch": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _vp]),
    # two parties: evaluation-only server, packed GLWE replies
    "fhe_import_eval_keys": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "fhe_pack_key_words": (C.c_size_t, [C.POINTER(fhe_params), _i32, _i32]),
    "fhe_pack_plan": (C.c_int, [C.POINTER(fhe_params), _i64, C.c_double, C.POINTER(_i32), C.POINTER(_i32),
                                C.POINTER(_i32)]),
    "fhe_keygen_pack_key_key": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "fhe_keygen_pack_key": (C.c_int, [_vp, _i32, _i32, _u64, _vp]),
    "fhe_export_pack_key": (C.c_int, [_vp, _vp]),
    "fhe_import_pack_key": (C.c_int, [_vp, _i32, _i32, _vp]),
    "fhe_pack_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "fhe_decrypt_packed_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "fhe_search_query_batch": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    # several queries of one key holder in one pass
    "fhe_linear_queries_batch": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "fhe_compare_queries_batch": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp,
                                            _vp]),
    "fhe_search_queries_batch": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp,
                                           _vp]),
    # stored-ciphertext search, several clear queries in one pass
    "fhe_linear_seeded_queries_batch": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "fhe_compare_seeded_queries_batch": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                                   _vp]),
    "fhe_search_seeded_queries_batch": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i32, _vp,
                                                  _vp, _vp]),
    # stored-ciphertext key rotation: the bridge key switch
    "fhe_bridge_key_words": (C.c_size_t, [C.POINTER(fhe_params), _i32, _i32]),
    "fhe_bridge_plan": (C.c_int, [C.POINTER(fhe_params), C.c_double, C.POINTER(_i32), C.POINTER(_i32)]),
    "fhe_keygen_bridge_key_key": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "fhe_export_bridge_key": (C.c_int, [_vp, _vp]),
    "fhe_import_bridge_key": (C.c_int, [_vp, _i32, _i32, _vp]),
    "fhe_bridge_batch": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "fhe_search_seeded_queries_bridged_batch": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i32,
                                                          _i64, _vp, _vp, _vp]),
    # several old generations resident: bridge slots and the generation row map
    "fhe_keygen_bridge_key_slot_key": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "fhe_export_bridge_key_slot": (C.c_int, [_vp, _i32, _vp]),
    "fhe_import_bridge_key_slot": (C.c_int, [_vp, _i32, _i32, _i32, _vp]),
    "fhe_import_bridge_key_slot_seeded": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "fhe_drop_bridge_key_slot": (C.c_int, [_vp, _i32]),
    "fhe_bridge_gens_batch": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "fhe_search_seeded_queries_gens_batch": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i32,
                                                       _i32, _vp, _vp, _vp, _vp, _vp]),
    # both sides encrypted: GGSW query x GLWE documents
    "fhe_encrypt_packed_batch_key": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _u64, _vp, _vp]),
    "fhe_encrypt_packed_batch": (C.c_int, [_vp, _vp, _i64, _i32, _u64, _u64, _vp, _vp]),
    "fhe_ggsw_words": (C.c_size_t, [C.POINTER(fhe_params), _i32, _i32]),
    "fhe_encrypt_ggsw_key": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _u64, _vp, _vp]),
    "fhe_encrypt_ggsw": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _u64, _u64, _vp, _vp]),
    "fhe_extprod_plan": (C.c_int, [C.POINTER(fhe_params), C.c_double, C.POINTER(_i32), C.POINTER(_i32)]),
    "fhe_glwe_docs_bytes": (C.c_size_t, [C.POINTER(fhe_params), _i64, _i32, _i32]),
    "fhe_glwe_docs_pack": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "fhe_linear_ggsw_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _i32, _i64, _vp, _vp]),
    "fhe_compare_ggsw_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp]),
    "fhe_search_ggsw_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _vp, _vp, _vp]),
    # several GGSW queries in one pass
    "fhe_glwe_docs_queries_bytes": (C.c_size_t, [C.POINTER(fhe_params), _i64, _i32, _i32]),
    "fhe_glwe_docs_queries_pack": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "fhe_ggsws_ws_bytes": (C.c_size_t, [C.POINTER(fhe_params), _i64, _i64, _i32, _i32]),
    "fhe_linear_ggsws_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "fhe_compare_ggsws_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    "fhe_search_ggsws_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _i64, _i32, _i64, _vp, _i32, _vp, _vp,
                                         _vp]),
    # both sides encrypted, after a key rotation: per-generation queries, one bridge
    "fhe_ggsws_gens_ws_bytes": (C.c_size_t, [C.POINTER(fhe_params), _i64, _vp, _i32, _i32, _i32]),
    "fhe_linear_ggsws_gens_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _i32, _vp, _vp, _vp]),
    "fhe_search_ggsws_gens_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp]),
    # both sides encrypted, seeded documents and queries
    "fhe_ggsw_body_words": (C.c_size_t, [C.POINTER(fhe_params), _i32, _i32]),
    "fhe_encrypt_packed_seeded_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _u64, _vp, _vp]),
    "fhe_encrypt_ggsw_seeded": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp]),
    "fhe_expand_packed_seeded_batch": (C.c_int, [_vp, _vp, _u64, _i64, _i32, _vp, _vp, _vp]),
    "fhe_expand_ggsws_seeded": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "fhe_glwe_docs_pack_seeded": (C.c_int, [_vp, _vp, _u64, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "fhe_glwe_docs_queries_pack_seeded": (C.c_int, [_vp, _vp, _u64, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "fhe_search_ggsw_seeded_batch": (C.c_int, [_vp, _vp, _u64, _i32, _i32, _vp, _vp, _i64, _i32, _i64, _i64, _i32,
                                               _vp, _vp, _vp]),
    "fhe_search_ggsws_seeded_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _i64, _i32, _i64, _vp,
                                                _i32, _vp, _vp, _vp]),
    # seeded evaluation keys: bodies and public mask keys
    "fhe_bsk_body_words": (C.c_size_t, [C.POINTER(fhe_params)]),
    "fhe_ksk_body_words": (C.c_size_t, [C.POINTER(fhe_params)]),
    "fhe_fast_bsk_body_words": (C.c_size_t, [C.POINTER(fhe_params), _i32]),
    "fhe_pack_key_body_words": (C.c_size_t, [C.POINTER(fhe_params), _i32, _i32]),
    "fhe_bridge_key_body_words": (C.c_size_t, [C.POINTER(fhe_params), _i32, _i32]),
    "fhe_import_eval_keys_seeded": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "fhe_import_pack_key_seeded": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "fhe_import_bridge_key_seeded": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
}


def _key32() -> C.Array:
    """A 256-bit ChaCha20 key (8 u32 words) from the OS CSPRNG."""
    return (C.c_uint32 * 8).from_buffer_copy(os.urandom(32))


class GpuCompare:
    """One device context + keys; batched encrypted compares from numpy."""

    def __init__(self, params: dict, key_seed: int | None = None, device: int = 0, lib_path: str | None = None,
                 enc_seed: int | None = None):
        path = lib_path or os.environ.get("FHEICP_LIB", "libfheicp.so")
        self.L = L = C.CDLL(path)
        for name, (res, args) in _PROTOS.items():
            getattr(L, name).restype = res
            getattr(L, name).argtypes = args
        self.P = fhe_params(struct_size=C.sizeof(fhe_params), **{f: int(params.get(f, 0)) for f in FIELDS})
        self.ctx = _vp()
        self._ok(L.fhe_ctx_create(C.byref(self.P), device, C.byref(self.ctx)))
        if key_seed is None:
            self._ok(L.fhe_keygen_key(self.ctx, _key32(), None))
        else:
            self._ok(L.fhe_keygen(self.ctx, key_seed, None))  # 64-bit seed: tests only
        # the session's encryption stream: its own 256-bit key and a random id
        # start (enc_seed: the seeded test form, ids from 0)
        self.enc_seed = enc_seed
        self.enc_key = None if enc_seed is not None else _key32()
        self.next_id = 0 if enc_seed is not None else int.from_bytes(os.urandom(8), "little")

    def _take_ids(self, count: int) -> int:
        id0 = self.next_id
        self.next_id = (self.next_id + count) & 0xFFFFFFFFFFFFFFFF
        return id0

    def _ok(self, rc: int) -> None:
        if rc != 0:
            msg = self.L.fhe_last_error(self.ctx if self.ctx else None)
            raise RuntimeError(f"libfheicp error {rc}: {msg.decode() if msg else ''}")

    def _to_dev(self, a: np.ndarray) -> _vp:
        a = np.ascontiguousarray(a)
        d = _vp()
        self._ok(self.L.fhe_dev_alloc(self.ctx, a.nbytes, C.byref(d)))
        self._ok(self.L.fhe_memcpy_h2d(self.ctx, d, a.ctypes.data, a.nbytes, None))
        return d

    def _alloc(self, nbytes: int) -> _vp:
        d = _vp()
        self._ok(self.L.fhe_dev_alloc(self.ctx, nbytes, C.byref(d)))
        return d

    def _to_host(self, d: _vp, count: int) -> np.ndarray:
        out = np.empty(count, np.int64)
        self._ok(self.L.fhe_memcpy_d2h(self.ctx, out.ctypes.data, d, out.nbytes, None))
        return out

    def compare(self, q_x: np.ndarray, q_w: np.ndarray, cst: int, T: int):
        """Encrypted compare of B quantized feature rows: (acc int64[B], below int64[B])."""
        q_x = np.asarray(q_x, np.int64)
        B, D = q_x.shape
        bufs = [self._to_dev(q_x), self._to_dev(np.asarray(q_w, np.int64)), self._alloc(8 * B), self._alloc(8 * B)]
        try:
            id0 = self._take_ids(B * D)
            if self.enc_key is not None:
                rc = self.L.fhe_compare_batch_key(self.ctx, bufs[0], B, D, bufs[1], int(cst), int(T), self.enc_key,
                                                  id0, bufs[2], bufs[3], None)
            else:
                rc = self.L.fhe_compare_batch(self.ctx, bufs[0], B, D, bufs[1], int(cst), int(T), self.enc_seed,
                                              id0, bufs[2], bufs[3], None)
            self._ok(rc)
            return self._to_host(bufs[2], B), self._to_host(bufs[3], B)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def score(self, q_x: np.ndarray, q_w: np.ndarray, cst: int, centre: int):
        """The reference's own encrypted predict (fhe_similarity.py:151,
        predict(fhe="execute")): packed encryption + leveled dot + decryption,
        no bootstrap; the accumulators int64[B] (dequantize on the host).
        centre: the middle of the accumulator range, (lo + hi) // 2, so that
        acc - centre fits the msg_bits encoding."""
        q_x = np.asarray(q_x, np.int64)
        B, D = q_x.shape
        bufs = [self._to_dev(q_x), self._to_dev(np.asarray(q_w, np.int64)), self._alloc(8 * B)]
        try:
            id0 = self._take_ids(B * D)
            if self.enc_key is not None:
                rc = self.L.fhe_score_batch_key(self.ctx, bufs[0], B, D, bufs[1], int(cst), int(centre), self.enc_key,
                                                id0, bufs[2], None)
            else:
                rc = self.L.fhe_score_batch(self.ctx, bufs[0], B, D, bufs[1], int(cst), int(centre), self.enc_seed,
                                            id0, bufs[2], None)
            self._ok(rc)
            return self._to_host(bufs[2], B)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    # ---- private query: an encrypted query against clear documents ----------
    def pack_docs(self, dq: np.ndarray):
        """Quantized documents (int64 [B, D], values in [-128, 127]) -> the
        device-resident packed corpus (handle, B, D); free it with free_docs."""
        dq = np.asarray(dq, np.int64)
        B, D = dq.shape
        src = self._to_dev(dq)
        try:
            docs8 = self._alloc(self.L.fhe_query_docs_bytes(C.byref(self.P), B, D))
            self._ok(self.L.fhe_query_docs_pack(self.ctx, src, B, D, docs8, None))
            # fhe_memcpy_d2h synchronises the stream: the pack is done before src is freed
            self._to_host(src, 1)
        finally:
            self.L.fhe_dev_free(self.ctx, src)
        return docs8, B, D

    def free_docs(self, docs) -> None:
        self.L.fhe_dev_free(self.ctx, docs[0])

    def encrypt_query(self, qq: np.ndarray, mask_key, noise_key, id0: int | None = None):
        """Client side: the quantized query (int64 [D]) as one seeded row at
        the context's msg_bits; (body uint64 [D], id0). mask_key is public,
        noise_key secret (8 u32 words each)."""
        qq = np.asarray(qq, np.int64).reshape(1, -1)
        D = qq.shape[1]
        id0 = int.from_bytes(os.urandom(8), "little") if id0 is None else int(id0)
        bufs = [self._to_dev(qq), self._to_dev(np.array([id0], np.uint64)), self._alloc(8 * D)]
        try:
            mk = (C.c_uint32 * 8)(*[int(x) for x in mask_key])
            nk = (C.c_uint32 * 8)(*[int(x) for x in noise_key])
            self._ok(self.L.fhe_encrypt_seeded_batch(self.ctx, bufs[0], 1, D, mk, nk, bufs[1], bufs[2], None))
            return self._to_host(bufs[2], D).view(np.uint64), id0
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def compare_query(self, body: np.ndarray, id0: int, mask_key, docs, q_w: np.ndarray, cst: int, T: int):
        """Server side: the seeded query against a packed corpus (pack_docs):
        (acc int64[B], below int64[B]); w = q_w, T on the worst-case range."""
        docs8, B, D = docs
        bufs = [self._to_dev(np.asarray(body, np.uint64)), self._to_dev(np.asarray(q_w, np.int64)),
                self._alloc(8 * B), self._alloc(8 * B)]
        try:
            mk = (C.c_uint32 * 8)(*[int(x) for x in mask_key])
            self._ok(self.L.fhe_compare_query_batch(self.ctx, bufs[0], int(id0), mk, docs8, B, D, bufs[1], int(cst),
                                                    int(T), bufs[2], bufs[3], None))
            return self._to_host(bufs[2], B), self._to_host(bufs[3], B)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    # ---- two parties: packed replies -----------------------------------------
    def keygen_pack(self, count: int = 1024, in_var: float = 0.0, seed: int | None = None):
        """Key holder: plan (fhe_pack_plan) and generate the packing key;
        (base_log, level, bit_levels)."""
        b, lv, lb = _i32(), _i32(), _i32()
        self._ok(self.L.fhe_pack_plan(C.byref(self.P), count, in_var, C.byref(b), C.byref(lv), C.byref(lb)))
        if seed is None:
            self._ok(self.L.fhe_keygen_pack_key_key(self.ctx, b.value, lv.value, _key32(), None))
        else:
            self._ok(self.L.fhe_keygen_pack_key(self.ctx, b.value, lv.value, seed, None))  # tests only
        return b.value, lv.value, lb.value

    def search_query(self, body: np.ndarray, id0: int, mask_key, docs, q_w: np.ndarray, cst: int, T: int,
                     levels_bit: int = 0):
        """Server side without decryption: (glwe_acc, glwe_bit) uint64 host
        arrays of ceil(B / N) * (k+1) * N words each (the reply's two blocks)."""
        docs8, B, D = docs
        words = -(-B // self.P.N) * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(np.asarray(body, np.uint64)), self._to_dev(np.asarray(q_w, np.int64)),
                self._alloc(8 * words), self._alloc(8 * words)]
        try:
            mk = (C.c_uint32 * 8)(*[int(x) for x in mask_key])
            self._ok(self.L.fhe_search_query_batch(self.ctx, bufs[0], int(id0), mk, docs8, B, D, bufs[1], int(cst),
                                                   int(T), int(levels_bit), bufs[2], bufs[3], None))
            return self._to_host(bufs[2], words).view(np.uint64), self._to_host(bufs[3], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def decrypt_packed(self, glwe: np.ndarray, count: int, mode: int) -> np.ndarray:
        """Key holder: the first count coefficients of packed GLWEs; mode 0
        signed values, 1 bits, 2 raw phases."""
        bufs = [self._to_dev(np.asarray(glwe, np.uint64)), self._alloc(8 * count)]
        try:
            self._ok(self.L.fhe_decrypt_packed_batch(self.ctx, bufs[0], count, mode, bufs[1], None))
            return self._to_host(bufs[1], count)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    # ---- several queries of one key holder in one pass ---
    def compare_queries(self, bodies: np.ndarray, id0s, mask_key, docs, q_w: np.ndarray, cst: int, Ts):
        """Q seeded queries (bodies uint64 [Q, D], Q stream ids with disjoint
        ranges [id0, id0 + D), one mask key) against a packed corpus:
        (acc int64 [Q, B], below int64 [Q, B]); query q uses threshold Ts[q]."""
        docs8, B, D = docs
        bodies = np.ascontiguousarray(bodies, np.uint64).reshape(-1, D)
        Q = bodies.shape[0]
        hT = np.ascontiguousarray([int(t) for t in Ts], np.int64)
        bufs = [self._to_dev(bodies), self._to_dev(np.asarray(id0s, np.uint64).reshape(Q)),
                self._to_dev(np.asarray(q_w, np.int64)), self._alloc(8 * Q * B), self._alloc(8 * Q * B)]
        try:
            mk = (C.c_uint32 * 8)(*[int(x) for x in mask_key])
            self._ok(self.L.fhe_compare_queries_batch(self.ctx, bufs[0], bufs[1], mk, Q, docs8, B, D, bufs[2],
                                                      int(cst), hT.ctypes.data, bufs[3], bufs[4], None))
            return self._to_host(bufs[3], Q * B).reshape(Q, B), self._to_host(bufs[4], Q * B).reshape(Q, B)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def search_queries(self, bodies: np.ndarray, id0s, mask_key, docs, q_w: np.ndarray, cst: int, Ts,
                       levels_bit: int = 0):
        """Server side without decryption for Q queries: (glwe_acc, glwe_bit)
        uint64 host arrays of ceil(Q B / N) * (k+1) * N words each; result
        (q, b) is coefficient (q B + b) mod N of GLWE (q B + b) / N."""
        docs8, B, D = docs
        bodies = np.ascontiguousarray(bodies, np.uint64).reshape(-1, D)
        Q = bodies.shape[0]
        hT = np.ascontiguousarray([int(t) for t in Ts], np.int64)
        words = -(-(Q * B) // self.P.N) * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(bodies), self._to_dev(np.asarray(id0s, np.uint64).reshape(Q)),
                self._to_dev(np.asarray(q_w, np.int64)), self._alloc(8 * words), self._alloc(8 * words)]
        try:
            mk = (C.c_uint32 * 8)(*[int(x) for x in mask_key])
            self._ok(self.L.fhe_search_queries_batch(self.ctx, bufs[0], bufs[1], mk, Q, docs8, B, D, bufs[2],
                                                     int(cst), hT.ctypes.data, int(levels_bit), bufs[3], bufs[4],
                                                     None))
            return self._to_host(bufs[3], words).view(np.uint64), self._to_host(bufs[4], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    # ---- both sides encrypted: GGSW query x GLWE documents -------------------
    def ggsw_plan(self, w_norm2: float):
        """(base_log, level) of the query's GGSW for the worst-case squared
        norm of W = q_w * qq (fhe_extprod_plan); raises when no gadget keeps
        the margin at this msg_bits."""
        b, lv = _i32(), _i32()
        self._ok(self.L.fhe_extprod_plan(C.byref(self.P), float(w_norm2), C.byref(b), C.byref(lv)))
        return b.value, lv.value

    def encrypt_docs_glwe(self, dq: np.ndarray) -> np.ndarray:
        """Key holder: quantized documents (int64 [B, D], D <= N) -> the
        ceil(B / (N // D)) document GLWEs (uint64 host array)."""
        dq = np.asarray(dq, np.int64)
        B, D = dq.shape
        S = self.P.N // D
        G = -(-B // S)
        rows = np.zeros((G * S, D), np.int64)
        rows[:B] = dq
        words = G * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(rows), self._alloc(8 * words)]
        try:
            id0 = self._take_ids(G)
            if self.enc_key is not None:
                rc = self.L.fhe_encrypt_packed_batch_key(self.ctx, bufs[0], G, S * D, self.enc_key, id0, bufs[1], None)
            else:
                rc = self.L.fhe_encrypt_packed_batch(self.ctx, bufs[0], G, S * D, self.enc_seed, id0, bufs[1], None)
            self._ok(rc)
            return self._to_host(bufs[1], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def encrypt_ggsw(self, W: np.ndarray, base_log: int, level: int) -> np.ndarray:
        """Key holder: W_j = q_w[j] * qq_j (int64 [D]) -> the query's GGSW
        (uint64 host array of fhe_ggsw_words words)."""
        W = np.asarray(W, np.int64).reshape(-1)
        words = self.L.fhe_ggsw_words(C.byref(self.P), base_log, level)
        bufs = [self._to_dev(W), self._alloc(8 * words)]
        try:
            id0 = self._take_ids((self.P.k + 1) * level * self.P.k)
            if self.enc_key is not None:
                rc = self.L.fhe_encrypt_ggsw_key(self.ctx, bufs[0], W.size, base_log, level, self.enc_key, id0,
                                                 bufs[1], None)
            else:
                rc = self.L.fhe_encrypt_ggsw(self.ctx, bufs[0], W.size, base_log, level, self.enc_seed, id0, bufs[1],
                                             None)
            self._ok(rc)
            return self._to_host(bufs[1], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def pack_docs_glwe(self, glwe: np.ndarray, B: int, D: int, base_log: int, level: int):
        """Server: document GLWEs -> the device-resident digit operand
        (handle, B, D); free it with free_docs."""
        src = self._to_dev(np.asarray(glwe, np.uint64))
        try:
            docs8 = self._alloc(self.L.fhe_glwe_docs_bytes(C.byref(self.P), B, D, level))
            self._ok(self.L.fhe_glwe_docs_pack(self.ctx, src, B, D, base_log, level, docs8, None))
            self._to_host(docs8, 1)  # fhe_memcpy_d2h synchronises: the pack is done before src is freed
            return docs8, B, D
        finally:
            self.L.fhe_dev_free(self.ctx, src)

    def compare_ggsw(self, ggsw: np.ndarray, base_log: int, level: int, docs, cst: int, T: int):
        """Single party: (acc, below) of the GGSW query against packed
        encrypted documents (fhe_compare_ggsw_batch)."""
        docs8, B, D = docs
        bufs = [self._to_dev(np.asarray(ggsw, np.uint64)), self._alloc(8 * B), self._alloc(8 * B)]
        try:
            self._ok(self.L.fhe_compare_ggsw_batch(self.ctx, bufs[0], base_log, level, docs8, B, D, int(cst), int(T),
                                                   bufs[1], bufs[2], None))
            return self._to_host(bufs[1], B), self._to_host(bufs[2], B)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def search_ggsw(self, ggsw: np.ndarray, base_log: int, level: int, docs, cst: int, T: int, levels_bit: int = 0):
        """Untrusted host: (glwe_acc, glwe_bit) as search_query's
        (fhe_search_ggsw_batch; evaluation keys and the packing key only)."""
        docs8, B, D = docs
        words = -(-B // self.P.N) * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(np.asarray(ggsw, np.uint64)), self._alloc(8 * words), self._alloc(8 * words)]
        try:
            self._ok(self.L.fhe_search_ggsw_batch(self.ctx, bufs[0], base_log, level, docs8, B, D, int(cst), int(T),
                                                  int(levels_bit), bufs[1], bufs[2], None))
            return self._to_host(bufs[1], words).view(np.uint64), self._to_host(bufs[2], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    # ---- several GGSW queries in one pass ----------------
    def pack_docs_glwe_queries(self, glwe: np.ndarray, B: int, D: int, base_log: int, level: int):
        """Server: document GLWEs -> the device-resident operand of the
        batched calls (handle, B, D); free it with free_docs."""
        src = self._to_dev(np.asarray(glwe, np.uint64))
        try:
            docs = self._alloc(self.L.fhe_glwe_docs_queries_bytes(C.byref(self.P), B, D, level))
            self._ok(self.L.fhe_glwe_docs_queries_pack(self.ctx, src, B, D, base_log, level, docs, None))
            self._to_host(docs, 1)  # fhe_memcpy_d2h synchronises: the pack is done before src is freed
            return docs, B, D
        finally:
            self.L.fhe_dev_free(self.ctx, src)

    def _ggsws(self, ggsws, base_log: int, level: int):
        g = np.ascontiguousarray(ggsws, np.uint64).reshape(-1)
        words = self.L.fhe_ggsw_words(C.byref(self.P), base_log, level)
        if words == 0 or g.size == 0 or g.size % words:
            raise ValueError(f"{g.size} words are no whole number of GGSWs of gadget ({base_log}, {level})")
        return g, g.size // words

    def compare_ggsws(self, ggsws, base_log: int, level: int, docs, cst: int, Ts):
        """Single party: Q GGSW queries (uint64 [Q, fhe_ggsw_words]) against
        documents packed by pack_docs_glwe_queries: (acc int64 [Q, B], below
        int64 [Q, B]); query q uses threshold Ts[q] (fhe_compare_ggsws_batch)."""
        d, B, D = docs
        g, Q = self._ggsws(ggsws, base_log, level)
        hT = np.ascontiguousarray([int(t) for t in Ts], np.int64)
        if hT.size != Q:
            raise ValueError(f"{hT.size} thresholds for {Q} queries")
        bufs = [self._to_dev(g), self._alloc(8 * Q * B), self._alloc(8 * Q * B)]
        try:
            self._ok(self.L.fhe_compare_ggsws_batch(self.ctx, bufs[0], base_log, level, d, Q, B, D, int(cst),
                                                    hT.ctypes.data, bufs[1], bufs[2], None))
            return self._to_host(bufs[1], Q * B).reshape(Q, B), self._to_host(bufs[2], Q * B).reshape(Q, B)
        finally:
            for b in bufs:
                self.L.fhe_dev_free(self.ctx, b)

    def search_ggsws(self, ggsws, base_log: int, level: int, docs, cst: int, Ts, levels_bit: int = 0):
        """Untrusted host, Q GGSW queries: (glwe_acc, glwe_bit) uint64 host
        arrays of ceil(Q B / N) * (k+1) * N words each; result (q, b) is
        coefficient (q B + b) mod N of GLWE (q B + b) / N
        (fhe_search_ggsws_batch; evaluation keys and the packing key only)."""
        d, B, D = docs
        g, Q = self._ggsws(ggsws, base_log, level)
        hT = np.ascontiguousarray([int(t) for t in Ts], np.int64)
        if hT.size != Q:
            raise ValueError(f"{hT.size} thresholds for {Q} queries")
        words = -(-(Q * B) // self.P.N) * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(g), self._alloc(8 * words), self._alloc(8 * words)]
        try:
            self._ok(self.L.fhe_search_ggsws_batch(self.ctx, bufs[0], base_log, level, d, Q, B, D, int(cst),
                                                   hT.ctypes.data, int(levels_bit), bufs[1], bufs[2], None))
            return self._to_host(bufs[1], words).view(np.uint64), self._to_host(bufs[2], words).view(np.uint64)
        finally:
            for b in bufs:
                self.L.fhe_dev_free(self.ctx, b)

    # ---- seeded documents and queries ----------------------
    # mask_key: PUBLIC, travels with the payload; noise_key: SECRET, stays with
    # the key holder (both 8 u32 words, e.g. _key32()); never the same key.
    @staticmethod
    def _k8(key) -> C.Array:
        return (C.c_uint32 * 8)(*[int(x) for x in np.asarray(key, np.uint32).reshape(8)])

    def encrypt_docs_glwe_seeded(self, dq: np.ndarray, mask_key, noise_key, id0: int | None = None):
        """Key holder: quantized documents (int64 [B, D]) -> (bodies uint64
        [G N], id0): N words per document GLWE instead of (k+1) N."""
        dq = np.asarray(dq, np.int64)
        B, D = dq.shape
        S = self.P.N // D
        G = -(-B // S)
        rows = np.zeros((G * S, D), np.int64)
        rows[:B] = dq
        bufs = [self._to_dev(rows), self._alloc(8 * G * self.P.N)]
        try:
            id0 = self._take_ids(G) if id0 is None else int(id0)
            self._ok(self.L.fhe_encrypt_packed_seeded_batch(self.ctx, bufs[0], G, S * D, self._k8(mask_key),
                                                            self._k8(noise_key), id0, bufs[1], None))
            return self._to_host(bufs[1], G * self.P.N).view(np.uint64), id0
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def encrypt_ggsw_seeded(self, W: np.ndarray, base_log: int, level: int, mask_key, noise_key,
                            id0: int | None = None):
        """Key holder: W (int64 [D]) -> (bodies uint64 [fhe_ggsw_body_words], id0)."""
        W = np.asarray(W, np.int64).reshape(-1)
        words = self.L.fhe_ggsw_body_words(C.byref(self.P), base_log, level)
        bufs = [self._to_dev(W), self._alloc(8 * words)]
        try:
            id0 = self._take_ids((self.P.k + 1) * level * self.P.k) if id0 is None else int(id0)
            self._ok(self.L.fhe_encrypt_ggsw_seeded(self.ctx, bufs[0], W.size, base_log, level, self._k8(mask_key),
                                                    self._k8(noise_key), id0, bufs[1], None))
            return self._to_host(bufs[1], words).view(np.uint64), id0
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def expand_docs_glwe_seeded(self, bodies, id0: int, mask_key) -> np.ndarray:
        """Bodies -> the full-form document GLWEs (interop; fhe_expand_packed_seeded_batch)."""
        b = np.ascontiguousarray(bodies, np.uint64).reshape(-1)
        G, words = b.size // self.P.N, b.size * (self.P.k + 1)
        bufs = [self._to_dev(b), self._alloc(8 * words)]
        try:
            self._ok(self.L.fhe_expand_packed_seeded_batch(self.ctx, bufs[0], int(id0), G, self.P.N,
                                                           self._k8(mask_key), bufs[1], None))
            return self._to_host(bufs[1], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def expand_ggsws_seeded(self, bodies, id0s, base_log: int, level: int, mask_key) -> np.ndarray:
        """Q queries' bodies -> Q full-form GGSWs (fhe_expand_ggsws_seeded)."""
        b = np.ascontiguousarray(bodies, np.uint64).reshape(-1)
        ids = np.ascontiguousarray([int(i) for i in id0s], np.uint64)
        Q = ids.size
        words = Q * self.L.fhe_ggsw_words(C.byref(self.P), base_log, level)
        bufs = [self._to_dev(b), self._to_dev(ids), self._alloc(8 * words)]
        try:
            self._ok(self.L.fhe_expand_ggsws_seeded(self.ctx, bufs[0], bufs[1], Q, base_log, level,
                                                    self._k8(mask_key), bufs[2], None))
            return self._to_host(bufs[2], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def pack_docs_glwe_seeded(self, bodies, id0: int, mask_key, B: int, D: int, base_log: int, level: int,
                              queries: bool = False):
        """Server: seeded document bodies -> the device-resident operand
        (handle, B, D) of search_ggsw[_seeded] (fhe_glwe_docs_pack_seeded) or,
        with queries=True, of the batched calls
        (fhe_glwe_docs_queries_pack_seeded); free it with free_docs."""
        src = self._to_dev(np.ascontiguousarray(bodies, np.uint64))
        size = self.L.fhe_glwe_docs_queries_bytes if queries else self.L.fhe_glwe_docs_bytes
        pack = self.L.fhe_glwe_docs_queries_pack_seeded if queries else self.L.fhe_glwe_docs_pack_seeded
        try:
            docs = self._alloc(size(C.byref(self.P), B, D, level))
            self._ok(pack(self.ctx, src, int(id0), B, D, base_log, level, self._k8(mask_key), docs, None))
            self._to_host(docs, 1)  # fhe_memcpy_d2h synchronises: the pack is done before src is freed
            return docs, B, D
        finally:
            self.L.fhe_dev_free(self.ctx, src)

    def search_ggsw_seeded(self, body, id0: int, mask_key, base_log: int, level: int, docs, cst: int, T: int,
                           levels_bit: int = 0):
        """Untrusted host, one seeded query: search_ggsw's outputs (fhe_search_ggsw_seeded_batch)."""
        docs8, B, D = docs
        words = -(-B // self.P.N) * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(np.ascontiguousarray(body, np.uint64)), self._alloc(8 * words), self._alloc(8 * words)]
        try:
            self._ok(self.L.fhe_search_ggsw_seeded_batch(self.ctx, bufs[0], int(id0), base_log, level,
                                                         self._k8(mask_key), docs8, B, D, int(cst), int(T),
                                                         int(levels_bit), bufs[1], bufs[2], None))
            return self._to_host(bufs[1], words).view(np.uint64), self._to_host(bufs[2], words).view(np.uint64)
        finally:
            for d in bufs:
                self.L.fhe_dev_free(self.ctx, d)

    def search_ggsws_seeded(self, bodies, id0s, mask_key, base_log: int, level: int, docs, cst: int, Ts,
                            levels_bit: int = 0):
        """Untrusted host, Q seeded queries: search_ggsws' outputs (fhe_search_ggsws_seeded_batch)."""
        d, B, D = docs
        ids = np.ascontiguousarray([int(i) for i in id0s], np.uint64)
        hT = np.ascontiguousarray([int(t) for t in Ts], np.int64)
        Q = ids.size
        if hT.size != Q:
            raise ValueError(f"{hT.size} thresholds for {Q} queries")
        words = -(-(Q * B) // self.P.N) * (self.P.k + 1) * self.P.N
        bufs = [self._to_dev(np.ascontiguousarray(bodies, np.uint64)), self._to_dev(ids), self._alloc(8 * words),
                self._alloc(8 * words)]
        try:
            self._ok(self.L.fhe_search_ggsws_seeded_batch(self.ctx, bufs[0], bufs[1], base_log, level,
                                                          self._k8(mask_key), d, Q, B, D, int(cst), hT.ctypes.data,
                                                          int(levels_bit), bufs[2], bufs[3], None))
            return self._to_host(bufs[2], words).view(np.uint64), self._to_host(bufs[3], words).view(np.uint64)
        finally:
            for b in bufs:
                self.L.fhe_dev_free(self.ctx, b)

    def import_eval_keys_seeded(self, d: dict) -> None:
        """Untrusted host: replace this context's keys by a key holder's seeded
        evaluation keys (eval_mask_key, bsk_body, ksk_body, gadget_bsk{g}_body;
        pack_key_body / pack_mask_key / pack_gadget and the bridge key's three
        when present). The masks are regenerated on the device; the context
        holds no secret afterwards."""
        P = C.byref(self.P)

        def body(name, words):
            a = np.ascontiguousarray(d[name], np.uint64)
            if a.size != words or words == 0:
                raise ValueError(f"{name}: {a.size} words do not match these parameters ({words})")
            return a

        bsk, ksk = body("bsk_body", self.L.fhe_bsk_body_words(P)), body("ksk_body", self.L.fhe_ksk_body_words(P))
        gad = [body(f"gadget_bsk{g}_body", self.L.fhe_fast_bsk_body_words(P, g)) if f"gadget_bsk{g}_body" in d else None
               for g in (1, 2, 3, 4, 5)]
        ptrs = (_vp * 5)(*[a.ctypes.data if a is not None else None for a in gad])
        self._ok(self.L.fhe_import_eval_keys_seeded(self.ctx, self._k8(d["eval_mask_key"]), bsk.ctypes.data,
                                                    ksk.ctypes.data, ptrs))
        for name, words, imp in (("pack", self.L.fhe_pack_key_body_words, self.L.fhe_import_pack_key_seeded),
                                 ("bridge", self.L.fhe_bridge_key_body_words, self.L.fhe_import_bridge_key_seeded)):
            if f"{name}_key_body" in d:
                b, lv = (int(x) for x in np.asarray(d[f"{name}_gadget"]).reshape(2))
                a = body(f"{name}_key_body", words(P, b, lv))
                self._ok(imp(self.ctx, b, lv, self._k8(d[f"{name}_mask_key"]), a.ctypes.data))

    def close(self) -> None:
        if self.ctx:
            self.L.fhe_ctx_destroy(self.ctx)
            self.ctx = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
