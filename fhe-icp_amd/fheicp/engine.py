"""Device-side engine: one libfheicp context per GPU, torch tensors as buffers.

PyTorch is plumbing here (device allocation, streams, host<->device copies);
all arithmetic runs in the HIP kernels of libfheicp.so. Ciphertext words are
stored in int64 tensors (bit patterns of the u64 words).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .params import SchemeParams


def _ptr(t: torch.Tensor | None):
    if t is None:
        return None
    assert t.is_contiguous(), "buffers must be contiguous"
    return C.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Engine:
    """A TFHE context on one MI355X (gfx950) device."""

    def __init__(self, params: SchemeParams, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise _lib.FheError("fheicp.Engine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.params = params
        self._L = _lib.lib()
        self._P = _lib.params_struct(params.as_dict())
        h = C.c_void_p()
        _lib.check(self._L.fhe_ctx_create(C.byref(self._P), self.device.index, C.byref(h)))
        self._ctx = h
        self.big = params.k * params.N
        self.W = self.big + 1
        self.Ws = params.n + 1
        self.has_keys = False
        self.pack_gadget = None   # (base_log, level) of the packing key, once one is generated or imported
        self.bridge_gadget = None  # (base_log, level) of the bridge key (§8.12), once one is generated or imported
        self.slot_gadgets = {}     # the same for bridge slots 1.. (§8.17); slot 0 is bridge_gadget

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._L.fhe_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int) -> None:
        _lib.check(rc, self._ctx)

    def set_msg_bits(self, P: int) -> None:
        self._chk(self._L.fhe_set_msg_bits(self._ctx, int(P)))
        self.params = self.params.with_msg_bits(P)

    @property
    def msg_bits(self) -> int:
        return self.params.msg_bits

    # ---------------------------------------------------------------- keys --
    def keygen(self, seed: int | None = None, key=None, mask_key=None) -> None:
        """Generate the keys from a 256-bit ChaCha20 key (8 u32 words or 32
        bytes; fhe_keygen_key), or from a 64-bit seed (fhe_keygen: 64 bits of
        entropy, reproducible tests and benches only). Exactly one is given.
        With mask_key (a 256-bit key, or True for a fresh os.urandom one) the
        set is seeded (fhe_keygen_seeded): the masks come from
        the public mask key, secrets and noise from `key` (or the seed's key),
        and export_eval_keys(seeded=True) ships bodies and mask key alone."""
        if (seed is None) == (key is None):
            raise ValueError("keygen takes either a 64-bit seed or a 256-bit key")
        with torch.cuda.device(self.device):
            if mask_key is not None and mask_key is not False:
                noise = key if key is not None else self.key_from_seed(seed)
                self._chk(self._L.fhe_keygen_seeded(self._ctx, self._key(self._fresh(mask_key)), self._key(noise),
                                                    _stream(self.device)))
            elif key is not None:
                self._chk(self._L.fhe_keygen_key(self._ctx, self._key(key), _stream(self.device)))
            else:
                self._chk(self._L.fhe_keygen(self._ctx, C.c_uint64(seed), _stream(self.device)))
        self.has_keys = True

    def export_keys(self) -> dict:
        p = self.params
        out = {
            "s_small": np.zeros(p.n, np.uint64),
            "s_big": np.zeros(self.big, np.uint64),
            "bsk": np.zeros(self._L.fhe_bsk_words(C.byref(self._P)), np.uint64),
            "ksk": np.zeros(self._L.fhe_ksk_words(C.byref(self._P)), np.uint64),
        }
        self._chk(self._L.fhe_export_keys(self._ctx, *(C.c_void_p(out[k].ctypes.data)
                                                       for k in ("s_small", "s_big", "bsk", "ksk"))))
        return out

    def export_key(self, which: str) -> np.ndarray:
        """One array of export_keys() alone ("s_small", "s_big", "bsk" or "ksk")."""
        names = ("s_small", "s_big", "bsk", "ksk")
        sizes = (self.params.n, self.big, self._L.fhe_bsk_words(C.byref(self._P)),
                 self._L.fhe_ksk_words(C.byref(self._P)))
        out = np.zeros(sizes[names.index(which)], np.uint64)
        self._chk(self._L.fhe_export_keys(self._ctx, *(C.c_void_p(out.ctypes.data) if n == which else None
                                                       for n in names)))
        return out

    def export_fast_bsk(self, which: int = 1) -> np.ndarray:
        """Another gadget's bootstrapping key (which = 1: params.pbs_fast_*,
        2: pbs_fast2_*, 3: pbs_mid_*, 4: pbs_mid2_*, 5: pbs_mid0_*)."""
        from .params import gadget_level
        p = self.params
        if which not in (1, 2, 3, 4, 5) or not gadget_level(p, which):
            raise ValueError(f"these parameters have no fast gadget {which}")
        q = _lib.params_struct(p.as_dict())
        out = np.zeros(self._L.fhe_fast_bsk_words(C.byref(q), which), np.uint64)
        self._chk(self._L.fhe_export_fast_bsk(self._ctx, which, C.c_void_p(out.ctypes.data)))
        return out

    def import_keys(self, keys: dict) -> None:
        arrs = [np.ascontiguousarray(keys[k], dtype=np.uint64) for k in ("s_small", "s_big", "bsk", "ksk")]
        self._chk(self._L.fhe_import_keys(self._ctx, *(C.c_void_p(a.ctypes.data) for a in arrs)))
        self.has_keys = True

    # ------------------------------------------------------------- buffers --
    def empty_big(self, count: int) -> torch.Tensor:
        return torch.empty((count, self.W), dtype=torch.int64, device=self.device)

    def empty_small(self, count: int) -> torch.Tensor:
        return torch.empty((count, self.Ws), dtype=torch.int64, device=self.device)

    def to_dev(self, a, dtype=torch.int64) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            return a.to(self.device, dtype=dtype).contiguous()
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        return torch.from_numpy(a).to(self.device, dtype=dtype).contiguous()

    # ------------------------------------------------------ client / server --
    def encrypt(self, msg, seed: int, id0: int = 0) -> torch.Tensor:
        m = self.to_dev(msg).reshape(-1)
        ct = self.empty_big(m.numel())
        self._chk(self._L.fhe_encrypt_batch(self._ctx, _ptr(m), m.numel(), C.c_uint64(seed), C.c_uint64(id0),
                                            _ptr(ct), _stream(self.device)))
        return ct

    def decrypt(self, ct: torch.Tensor) -> torch.Tensor:
        n = ct.numel() // self.W
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_decrypt_batch(self._ctx, _ptr(ct), n, _ptr(out), _stream(self.device)))
        return out

    def decrypt_bits(self, ct: torch.Tensor) -> torch.Tensor:
        n = ct.numel() // self.W
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_decrypt_bits_batch(self._ctx, _ptr(ct), n, _ptr(out), _stream(self.device)))
        return out

    def phase(self, ct: torch.Tensor) -> torch.Tensor:
        n = ct.numel() // self.W
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_phase_batch(self._ctx, _ptr(ct), n, _ptr(out), _stream(self.device)))
        return out

    def linear(self, ct: torch.Tensor, B: int, D: int, w, cst: int) -> torch.Tensor:
        wd = self.to_dev(w)
        out = self.empty_big(B)
        self._chk(self._L.fhe_linear_batch(self._ctx, _ptr(ct), B, D, _ptr(wd), int(cst), _ptr(out),
                                           _stream(self.device)))
        return out

    def encrypt_linear(self, msg, w, cst: int, seed, id0: int = 0) -> torch.Tensor:
        """Fused encrypt + linear (fhe_encrypt_linear_batch[_key]): msg B x D
        ints; `seed` is an int seed (tests) or a 256-bit stream key."""
        m = self.to_dev(msg)
        B, D = m.shape
        wd = self.to_dev(w)
        out = self.empty_big(B)
        if isinstance(seed, (int, np.integer)):
            rc = self._L.fhe_encrypt_linear_batch(self._ctx, _ptr(m), B, D, C.c_uint64(int(seed)), C.c_uint64(id0),
                                                  _ptr(wd), int(cst), _ptr(out), _stream(self.device))
        else:
            rc = self._L.fhe_encrypt_linear_batch_key(self._ctx, _ptr(m), B, D, self._key(seed), C.c_uint64(id0),
                                                      _ptr(wd), int(cst), _ptr(out), _stream(self.device))
        self._chk(rc)
        return out

    def encrypt_packed(self, msg, seed: int, id0: int = 0) -> torch.Tensor:
        """Packed GLWE encryption of B x D features (fhe_encrypt_packed_batch):
        [B][ceil(D / N)][(k + 1) N] words."""
        m = self.to_dev(msg)
        B, D = m.shape
        p = self.params
        G = -(-D // p.N)
        out = torch.empty((B, G, (p.k + 1) * p.N), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_encrypt_packed_batch(self._ctx, _ptr(m), B, D, C.c_uint64(seed), C.c_uint64(id0),
                                                   _ptr(out), _stream(self.device)))
        return out

    def linear_packed(self, glwe: torch.Tensor, D: int, w, cst: int) -> torch.Tensor:
        """Leveled dot product on packed GLWE inputs (fhe_linear_packed_batch)."""
        B = glwe.shape[0]
        wd = self.to_dev(w)
        out = self.empty_big(B)
        self._chk(self._L.fhe_linear_packed_batch(self._ctx, _ptr(glwe), B, D, _ptr(wd), int(cst), _ptr(out),
                                                  _stream(self.device)))
        return out

    def keyswitch(self, ct: torch.Tensor, shift: int = 0, add_body: int = 0) -> torch.Tensor:
        n = ct.numel() // self.W
        out = self.empty_small(n)
        self._chk(self._L.fhe_keyswitch_batch(self._ctx, _ptr(ct), n, shift, C.c_uint64(add_body), _ptr(out),
                                              _stream(self.device)))
        return out

    def pbs(self, small: torch.Tensor, tv: int) -> torch.Tensor:
        n = small.numel() // self.Ws
        out = self.empty_big(n)
        self._chk(self._L.fhe_pbs_batch(self._ctx, _ptr(small), n, C.c_uint64(tv), _ptr(out), _stream(self.device)))
        return out

    def pbs_gadget(self, small: torch.Tensor, gadget: int, tv: int) -> torch.Tensor:
        """fhe_pbs_batch on gadget 0 (main), 1 (fast) or 2 (fast2) (fhe_pbs_gadget_batch)."""
        n = small.numel() // self.Ws
        out = self.empty_big(n)
        self._chk(self._L.fhe_pbs_gadget_batch(self._ctx, _ptr(small), n, int(gadget), C.c_uint64(tv), _ptr(out),
                                               _stream(self.device)))
        return out

    def pbs_lut(self, small: torch.Tensor, base: int, step: int, log_slots: int) -> torch.Tensor:
        """Staircase bootstrap (fhe_pbs_lut_batch)."""
        n = small.numel() // self.Ws
        out = self.empty_big(n)
        self._chk(self._L.fhe_pbs_lut_batch(self._ctx, _ptr(small), n, C.c_uint64(base), C.c_uint64(step),
                                            int(log_slots), _ptr(out), _stream(self.device)))
        return out

    def pbs_table(self, small: torch.Tensor, lut, lut_bits: int, gadget: int | None = None) -> torch.Tensor:
        """Table bootstrap (fhe_pbs_table_batch; fhe_pbs_table_gadget_batch
        with an explicit gadget): input m in [0, 2^lut_bits) at
        2^(63 - lut_bits); output lut[m] at 2^(64 - msg_bits)."""
        n = small.numel() // self.Ws
        lut_d = self.to_dev(np.asarray(lut, dtype=np.int64)) if not isinstance(lut, torch.Tensor) else lut
        out = self.empty_big(n)
        if gadget is None:
            rc = self._L.fhe_pbs_table_batch(self._ctx, _ptr(small), n, _ptr(lut_d), int(lut_bits), _ptr(out),
                                             _stream(self.device))
        else:
            rc = self._L.fhe_pbs_table_gadget_batch(self._ctx, _ptr(small), n, int(gadget), _ptr(lut_d),
                                                    int(lut_bits), _ptr(out), _stream(self.device))
        self._chk(rc)
        return out

    def table_gadget(self) -> int:
        """The gadget fhe_pbs_table_batch runs on (fhe_pbs_table_gadget)."""
        return self._L.fhe_pbs_table_gadget(C.byref(self._P_now()))

    def threshold(self, ct_acc: torch.Tensor, T: int) -> torch.Tensor:
        """Encryption of [acc >= T] at 2^63 (fhe_threshold_batch); ct_acc is kept."""
        n = ct_acc.numel() // self.W
        bit = self.empty_big(n)
        self._chk(self._L.fhe_threshold_batch(self._ctx, _ptr(ct_acc), n, int(T), _ptr(bit), _stream(self.device)))
        return bit

    def sign(self, ct_v: torch.Tensor) -> torch.Tensor:
        """Consumes ct_v; returns the encryption of [v < 0] at 2^63 (fhe_sign_batch)."""
        n = ct_v.numel() // self.W
        sign = self.empty_big(n)
        self._chk(self._L.fhe_sign_batch(self._ctx, _ptr(ct_v), n, _ptr(sign), _stream(self.device)))
        return sign

    def sign_trace(self, ct_v: torch.Tensor, sched=None, rounds: int = 0, phases: bool = True):
        """Measurement only (fhe_sign_trace_batch): consumes ct_v and runs the
        sign extraction's rounds (all, or the first `rounds`) on an explicit
        gadget schedule (None: the plan's). Returns (sign ciphertexts or None,
        phases uint32 tensor [R][count] of every round's rotation exponent or
        None)."""
        n = ct_v.numel() // self.W
        R = len(sched) if sched is not None else None
        if R is None:
            cap = (C.c_int32 * 64)()
            R = self._L.fhe_sign_schedule(C.byref(self._P_now()), cap, 64)
            if R < 0:
                _lib.check(R)
        last = rounds in (0, R)
        sign = self.empty_big(n) if last else None
        ph = torch.empty((R, n), dtype=torch.int32, device=self.device) if phases else None
        hs = (C.c_int32 * R)(*[int(g) for g in sched]) if sched is not None else None
        self._chk(self._L.fhe_sign_trace_batch(self._ctx, _ptr(ct_v), n, hs, int(rounds), _ptr(sign), _ptr(ph),
                                               _stream(self.device)))
        return sign, ph

    def _P_now(self):
        return _lib.params_struct(self.params.as_dict())

    def bit_extract(self, ct_v: torch.Tensor):
        """Consumes ct_v; returns (refreshed, sign) ciphertexts."""
        n = ct_v.numel() // self.W
        ref = self.empty_big(n)
        sign = self.empty_big(n)
        self._chk(self._L.fhe_bit_extract_batch(self._ctx, _ptr(ct_v), n, _ptr(ref), _ptr(sign),
                                                _stream(self.device)))
        return ref, sign

    def compare(self, q_x: torch.Tensor, w: torch.Tensor, cst: int, T: int, enc, id0: int = 0):
        """Fused encrypt -> linear -> decrypt + sign extraction for B pairs.
        `enc` is the session's 256-bit stream key (8 u32 words or 32 bytes:
        fhe_compare_batch_key) or an int seed (fhe_compare_batch, tests).

        Returns (acc int64[B], below int64[B])."""
        B, D = q_x.shape
        acc = torch.empty(B, dtype=torch.int64, device=self.device)
        below = torch.empty(B, dtype=torch.int64, device=self.device)
        if isinstance(enc, (int, np.integer)):
            rc = self._L.fhe_compare_batch(self._ctx, _ptr(q_x), B, D, _ptr(w), int(cst), int(T), C.c_uint64(int(enc)),
                                           C.c_uint64(id0), _ptr(acc), _ptr(below), _stream(self.device))
        else:
            rc = self._L.fhe_compare_batch_key(self._ctx, _ptr(q_x), B, D, _ptr(w), int(cst), int(T), self._key(enc),
                                               C.c_uint64(id0), _ptr(acc), _ptr(below), _stream(self.device))
        self._chk(rc)
        return acc, below

    def score(self, q_x: torch.Tensor, w: torch.Tensor, cst: int, T: int, enc, id0: int = 0):
        """The leveled circuit alone (fhe_score_batch[_key]): encrypt -> linear
        -> decrypt, no key switch or bootstrap. T centres acc in the encoding;
        `enc` as in compare(). Returns acc int64[B]."""
        B, D = q_x.shape
        acc = torch.empty(B, dtype=torch.int64, device=self.device)
        if isinstance(enc, (int, np.integer)):
            rc = self._L.fhe_score_batch(self._ctx, _ptr(q_x), B, D, _ptr(w), int(cst), int(T), C.c_uint64(int(enc)),
                                         C.c_uint64(id0), _ptr(acc), _stream(self.device))
        else:
            rc = self._L.fhe_score_batch_key(self._ctx, _ptr(q_x), B, D, _ptr(w), int(cst), int(T), self._key(enc),
                                             C.c_uint64(id0), _ptr(acc), _stream(self.device))
        self._chk(rc)
        return acc

    # ------------------------------------------- seeded (stored) corpus --
    @staticmethod
    def key_from_seed(seed: int) -> np.ndarray:
        out = np.zeros(8, np.uint32)
        _lib.lib().fhe_key_from_seed(C.c_uint64(seed), C.c_void_p(out.ctypes.data))
        return out

    @staticmethod
    def _fresh(mask_key):
        """A mask key argument: True stands for a fresh 32 bytes of the OS CSPRNG."""
        if mask_key is True:
            import os
            return os.urandom(32)
        return mask_key

    @staticmethod
    def _key(k) -> C.Array:
        if isinstance(k, (bytes, bytearray)):
            if len(k) != 32:
                raise ValueError("a ChaCha20 key is 32 bytes")
            k = np.frombuffer(bytes(k), dtype="<u4")
        k = np.ascontiguousarray(k, dtype=np.uint32).reshape(8)
        return (C.c_uint32 * 8)(*[int(x) for x in k])

    def quantize(self, x: torch.Tensor, scale: float, zero_point: int, qmin: int, qmax: int) -> torch.Tensor:
        """clip(rint(x / scale + zp), qmin, qmax) of a device f32/f64 [B, D] (fhe_quantize_pairs)."""
        B, D = x.shape
        q = torch.empty((B, D), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_quantize_pairs(self._ctx, None, 0, _ptr(x), 1 if x.dtype == torch.float64 else 0, B, D,
                                             C.c_double(scale), int(zero_point), int(qmin), int(qmax), _ptr(q),
                                             _stream(self.device)))
        return q

    def encrypt_seeded(self, msg: torch.Tensor, mask_key, noise_key, id0: torch.Tensor) -> torch.Tensor:
        B, D = msg.shape
        body = torch.empty((B, D), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_encrypt_seeded_batch(self._ctx, _ptr(msg), B, D, self._key(mask_key),
                                                   self._key(noise_key), _ptr(id0), _ptr(body), _stream(self.device)))
        return body

    def expand_seeded(self, body: torch.Tensor, id0: torch.Tensor, B: int, D: int, mask_key) -> torch.Tensor:
        ct = self.empty_big(B * D)
        self._chk(self._L.fhe_expand_seeded_batch(self._ctx, _ptr(body), _ptr(id0), B, D, self._key(mask_key),
                                                  _ptr(ct), _stream(self.device)))
        return ct

    def linear_seeded(self, body: torch.Tensor, id0: torch.Tensor, mask_key, w, cst: int) -> torch.Tensor:
        B, D = body.shape
        wd = self.to_dev(w)
        out = self.empty_big(B)
        self._chk(self._L.fhe_linear_seeded_batch(self._ctx, _ptr(body), _ptr(id0), B, D, self._key(mask_key),
                                                  _ptr(wd), int(cst), _ptr(out), _stream(self.device)))
        return out

    def compare_seeded(self, body: torch.Tensor, id0: torch.Tensor, mask_key, w: torch.Tensor, cst: int, T: int):
        """fhe_compare_seeded_batch: (acc int64[B], below int64[B])."""
        B, D = body.shape
        acc = torch.empty(B, dtype=torch.int64, device=self.device)
        below = torch.empty(B, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_compare_seeded_batch(self._ctx, _ptr(body), _ptr(id0), B, D, self._key(mask_key),
                                                   _ptr(w), int(cst), int(T), _ptr(acc), _ptr(below),
                                                   _stream(self.device)))
        return acc, below

    # ------------------------- private query (encrypted query, clear docs) --
    def pack_docs(self, dq: torch.Tensor) -> torch.Tensor:
        """Quantized documents (int64 [B, D], values in [-128, 127]) -> the
        i8 MFMA document operand of linear_query / compare_query
        (fhe_query_docs_pack): a uint8 tensor of fhe_query_docs_bytes bytes."""
        B, D = dq.shape
        n = self._L.fhe_query_docs_bytes(C.byref(self._P), B, D)
        docs8 = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._chk(self._L.fhe_query_docs_pack(self._ctx, _ptr(dq), B, D, _ptr(docs8), _stream(self.device)))
        return docs8

    def linear_query(self, ct_q: torch.Tensor, docs8: torch.Tensor, B: int, D: int, w, cst: int) -> torch.Tensor:
        """out[b] = sum_j dq[b, j] * (w[j] * ct_q[j]) + cst (fhe_linear_query_batch):
        ct_q D x (kN+1), docs8 from pack_docs; B x (kN+1)."""
        wd = self.to_dev(w)
        out = self.empty_big(B)
        self._chk(self._L.fhe_linear_query_batch(self._ctx, _ptr(ct_q), _ptr(docs8), B, D, _ptr(wd), int(cst),
                                                 _ptr(out), _stream(self.device)))
        return out

    def compare_query(self, qbody: torch.Tensor, id0: int, mask_key, docs8: torch.Tensor, B: int, D: int,
                      w: torch.Tensor, cst: int, T: int):
        """fhe_compare_query_batch: a seeded query (D body words, stream id,
        public mask key) against packed clear documents;
        (acc int64[B], below int64[B])."""
        acc = torch.empty(B, dtype=torch.int64, device=self.device)
        below = torch.empty(B, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_compare_query_batch(self._ctx, _ptr(qbody), C.c_uint64(int(id0)), self._key(mask_key),
                                                  _ptr(docs8), B, D, _ptr(w), int(cst), int(T), _ptr(acc),
                                                  _ptr(below), _stream(self.device)))
        return acc, below

    # ------------------ two-party private query: evaluation keys, packing --
    def keygen_pack(self, base_log: int, level: int, key=None, seed: int | None = None, mask_key=None) -> None:
        """Generate the LWE -> GLWE packing key for gadget (base_log, level)
        (fhe_keygen_pack_key[_key]); `key` is a 256-bit ChaCha20 key (os.urandom
        when neither is given), `seed` the 64-bit test form. With mask_key (a
        256-bit key of this packing key alone, or True for a fresh one) the key
        is seeded (fhe_keygen_pack_key_seeded, §8.16): `key` / `seed` is the
        secret noise key."""
        if mask_key is not None and mask_key is not False:
            import os
            noise = self.key_from_seed(seed) if seed is not None else (key if key is not None else os.urandom(32))
            rc = self._L.fhe_keygen_pack_key_seeded(self._ctx, int(base_log), int(level),
                                                    self._key(self._fresh(mask_key)), self._key(noise),
                                                    _stream(self.device))
        elif seed is not None:
            rc = self._L.fhe_keygen_pack_key(self._ctx, int(base_log), int(level), C.c_uint64(seed),
                                             _stream(self.device))
        else:
            import os
            rc = self._L.fhe_keygen_pack_key_key(self._ctx, int(base_log), int(level),
                                                 self._key(key if key is not None else os.urandom(32)),
                                                 _stream(self.device))
        self._chk(rc)
        self.pack_gadget = (int(base_log), int(level))

    def export_pack_key(self) -> np.ndarray:
        b, L = self.pack_gadget
        out = np.zeros(self._L.fhe_pack_key_words(C.byref(self._P), b, L), np.uint64)
        self._chk(self._L.fhe_export_pack_key(self._ctx, C.c_void_p(out.ctypes.data)))
        return out

    def import_pack_key(self, base_log: int, level: int, key) -> None:
        a = np.ascontiguousarray(key, dtype=np.uint64)
        if a.size != self._L.fhe_pack_key_words(C.byref(self._P), int(base_log), int(level)):
            raise ValueError("packing key size does not match its gadget and these parameters")
        self._chk(self._L.fhe_import_pack_key(self._ctx, int(base_log), int(level), C.c_void_p(a.ctypes.data)))
        self.pack_gadget = (int(base_log), int(level))

    # ------- stored-ciphertext key rotation: the bridge key switch (§8.12) --
    def bridge_key_words(self, base_log: int, level: int) -> int:
        return int(self._L.fhe_bridge_key_words(C.byref(self._P), int(base_log), int(level)))

    def bridge_gadget_of(self, slot: int = 0):
        """(base_log, level) of the bridge key in `slot`, None for an empty slot."""
        return self.bridge_gadget if int(slot) == 0 else self.slot_gadgets.get(int(slot))

    def _set_bridge_gadget(self, slot: int, gadget) -> None:
        if int(slot) == 0:
            self.bridge_gadget = gadget
        elif gadget is None:
            self.slot_gadgets.pop(int(slot), None)
        else:
            self.slot_gadgets[int(slot)] = gadget

    def bridge_slots(self) -> list:
        """The bridge slots that hold a key, ascending."""
        return ([0] if self.bridge_gadget else []) + sorted(self.slot_gadgets)

    def keygen_bridge_key(self, s_big_old, base_log: int, level: int, key=None, seed: int | None = None,
                          mask_key=None, slot: int = 0) -> None:
        """Generate the bridge key from the old big key s_big_old (kN words of
        0/1, export_keys()["s_big"] of the old context) to this context's
        secret (fhe_keygen_bridge_key[_key]); `key` is a 256-bit ChaCha20 key
        (os.urandom when neither is given), `seed` the 64-bit test form. With
        mask_key (this bridge key's own, or True for a fresh one) the key is
        seeded (fhe_keygen_bridge_key_seeded, §8.16). slot > 0: into that
        bridge slot (the *_slot entries, §8.17)."""
        s = np.ascontiguousarray(s_big_old, dtype=np.uint64).reshape(-1)
        if s.size != self.big:
            raise ValueError(f"the old big key holds {s.size} words, these parameters {self.big}")
        sp = C.c_void_p(s.ctypes.data)
        slot = int(slot)
        at = (slot,) if slot else ()
        L = self._L
        if mask_key is not None and mask_key is not False:
            import os
            noise = self.key_from_seed(seed) if seed is not None else (key if key is not None else os.urandom(32))
            fn = L.fhe_keygen_bridge_key_slot_seeded if slot else L.fhe_keygen_bridge_key_seeded
            rc = fn(self._ctx, *at, sp, int(base_log), int(level), self._key(self._fresh(mask_key)), self._key(noise),
                    _stream(self.device))
        elif seed is not None:
            fn = L.fhe_keygen_bridge_key_slot if slot else L.fhe_keygen_bridge_key
            rc = fn(self._ctx, *at, sp, int(base_log), int(level), C.c_uint64(seed), _stream(self.device))
        else:
            import os
            fn = L.fhe_keygen_bridge_key_slot_key if slot else L.fhe_keygen_bridge_key_key
            rc = fn(self._ctx, *at, sp, int(base_log), int(level),
                    self._key(key if key is not None else os.urandom(32)), _stream(self.device))
        self._chk(rc)
        self._set_bridge_gadget(slot, (int(base_log), int(level)))

    def export_bridge_key(self, slot: int = 0) -> np.ndarray:
        slot = int(slot)
        if not self.bridge_gadget_of(slot):
            raise _lib.FheError("FHE_E_STATE: no bridge key" + (f" in slot {slot}" if slot else ""))
        out = np.zeros(self.bridge_key_words(*self.bridge_gadget_of(slot)), np.uint64)
        if slot:
            self._chk(self._L.fhe_export_bridge_key_slot(self._ctx, slot, C.c_void_p(out.ctypes.data)))
        else:
            self._chk(self._L.fhe_export_bridge_key(self._ctx, C.c_void_p(out.ctypes.data)))
        return out

    def import_bridge_key(self, base_log: int, level: int, key, slot: int = 0) -> None:
        a = np.ascontiguousarray(key, dtype=np.uint64)
        if a.size != self.bridge_key_words(base_log, level):
            raise ValueError("bridge key size does not match its gadget and these parameters")
        slot = int(slot)
        if slot:
            self._chk(self._L.fhe_import_bridge_key_slot(self._ctx, slot, int(base_log), int(level),
                                                         C.c_void_p(a.ctypes.data)))
        else:
            self._chk(self._L.fhe_import_bridge_key(self._ctx, int(base_log), int(level), C.c_void_p(a.ctypes.data)))
        self._set_bridge_gadget(slot, (int(base_log), int(level)))

    def drop_bridge_key(self, slot: int) -> None:
        """fhe_drop_bridge_key_slot: frees the slot's key (an empty slot: nothing to do)."""
        self._chk(self._L.fhe_drop_bridge_key_slot(self._ctx, int(slot)))
        self._set_bridge_gadget(int(slot), None)

    def bridge(self, ct: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Big LWEs under the old key -> under this context's key
        (fhe_bridge_batch); out may be ct."""
        n = ct.numel() // self.W
        if out is None:
            out = self.empty_big(n)
        self._chk(self._L.fhe_bridge_batch(self._ctx, _ptr(ct), n, _ptr(out), _stream(self.device)))
        return out

    def bridge_rows(self, ct: torch.Tensor, Q: int, B: int, b_old: int) -> torch.Tensor:
        """fhe_bridge_rows_batch: in place on rows {q B + b : b < b_old} of a
        query-major Q x B result."""
        if ct.numel() < int(Q) * int(B) * self.W:
            raise ValueError(f"{ct.numel() // self.W} ciphertexts for {Q} x {B} rows")
        self._chk(self._L.fhe_bridge_rows_batch(self._ctx, _ptr(ct), int(Q), int(B), int(b_old),
                                                _stream(self.device)))
        return ct

    @staticmethod
    def _gens(ends, slots):
        """The generation row map as host tables: (G, int64[G], int32[G])."""
        ends, slots = [int(e) for e in ends], [int(s) for s in slots]
        if len(ends) != len(slots):
            raise ValueError(f"{len(ends)} generation ends for {len(slots)} bridge slots")
        G = len(ends)
        return G, (C.c_int64 * max(G, 1))(*ends), (C.c_int32 * max(G, 1))(*slots)

    def bridge_gens(self, ct: torch.Tensor, Q: int, B: int, ends, slots) -> torch.Tensor:
        """fhe_bridge_gens_batch: in place on a query-major Q x B result whose
        documents ends[g - 1] <= b < ends[g] are under old generation g,
        bridged by slot slots[g] (§8.17)."""
        if ct.numel() < int(Q) * int(B) * self.W:
            raise ValueError(f"{ct.numel() // self.W} ciphertexts for {Q} x {B} rows")
        G, he, hs = self._gens(ends, slots)
        self._chk(self._L.fhe_bridge_gens_batch(self._ctx, _ptr(ct), int(Q), int(B), G, he, hs,
                                                _stream(self.device)))
        return ct

    def export_pack_key_seeded(self):
        """(mask key u32[8], bodies) of a seeded packing key (fhe_export_pack_key_seeded)."""
        b, L = self.pack_gadget
        mk = np.zeros(8, np.uint32)
        out = np.zeros(self._L.fhe_pack_key_body_words(C.byref(self._P), b, L), np.uint64)
        self._chk(self._L.fhe_export_pack_key_seeded(self._ctx, C.c_void_p(mk.ctypes.data),
                                                     C.c_void_p(out.ctypes.data)))
        return mk, out

    def import_pack_key_seeded(self, base_log: int, level: int, mask_key, body) -> None:
        a = np.ascontiguousarray(body, dtype=np.uint64)
        if a.size != self._L.fhe_pack_key_body_words(C.byref(self._P), int(base_log), int(level)):
            raise ValueError("pack_key_body: size does not match its gadget and these parameters")
        self._chk(self._L.fhe_import_pack_key_seeded(self._ctx, int(base_log), int(level), self._key(mask_key),
                                                     C.c_void_p(a.ctypes.data)))
        self.pack_gadget = (int(base_log), int(level))

    def export_bridge_key_seeded(self, slot: int = 0):
        """(mask key u32[8], bodies) of a seeded bridge key (fhe_export_bridge_key_seeded)."""
        slot = int(slot)
        if not self.bridge_gadget_of(slot):
            raise _lib.FheError("FHE_E_STATE: no bridge key" + (f" in slot {slot}" if slot else ""))
        mk = np.zeros(8, np.uint32)
        out = np.zeros(self._L.fhe_bridge_key_body_words(C.byref(self._P), *self.bridge_gadget_of(slot)), np.uint64)
        if slot:
            self._chk(self._L.fhe_export_bridge_key_slot_seeded(self._ctx, slot, C.c_void_p(mk.ctypes.data),
                                                                C.c_void_p(out.ctypes.data)))
        else:
            self._chk(self._L.fhe_export_bridge_key_seeded(self._ctx, C.c_void_p(mk.ctypes.data),
                                                           C.c_void_p(out.ctypes.data)))
        return mk, out

    def import_bridge_key_seeded(self, base_log: int, level: int, mask_key, body, slot: int = 0) -> None:
        a = np.ascontiguousarray(body, dtype=np.uint64)
        if a.size != self._L.fhe_bridge_key_body_words(C.byref(self._P), int(base_log), int(level)):
            raise ValueError("bridge_key_body: size does not match its gadget and these parameters")
        slot = int(slot)
        if slot:
            self._chk(self._L.fhe_import_bridge_key_slot_seeded(self._ctx, slot, int(base_log), int(level),
                                                                self._key(mask_key), C.c_void_p(a.ctypes.data)))
        else:
            self._chk(self._L.fhe_import_bridge_key_seeded(self._ctx, int(base_log), int(level), self._key(mask_key),
                                                           C.c_void_p(a.ctypes.data)))
        self._set_bridge_gadget(slot, (int(base_log), int(level)))

    def _export_eval_keys_seeded(self) -> dict:
        from .params import gadget_level
        p = self.params
        out = {"eval_mask_key": np.zeros(8, np.uint32),
               "bsk_body": np.zeros(self._L.fhe_bsk_body_words(C.byref(self._P)), np.uint64),
               "ksk_body": np.zeros(self._L.fhe_ksk_body_words(C.byref(self._P)), np.uint64)}
        for g in (1, 2, 3, 4, 5):
            if gadget_level(p, g):
                out[f"gadget_bsk{g}_body"] = np.zeros(self._L.fhe_fast_bsk_body_words(C.byref(self._P), g), np.uint64)
        ptrs = (C.c_void_p * 5)(*[out[f"gadget_bsk{g}_body"].ctypes.data if f"gadget_bsk{g}_body" in out else None
                                  for g in (1, 2, 3, 4, 5)])
        self._chk(self._L.fhe_export_eval_keys_seeded(self._ctx, C.c_void_p(out["eval_mask_key"].ctypes.data),
                                                      C.c_void_p(out["bsk_body"].ctypes.data),
                                                      C.c_void_p(out["ksk_body"].ctypes.data), ptrs))
        if self.pack_gadget:
            out["pack_mask_key"], out["pack_key_body"] = self.export_pack_key_seeded()
            out["pack_gadget"] = np.array(self.pack_gadget, dtype=np.int64)
        self._export_bridges(out, True)
        return out

    def _export_bridges(self, out: dict, seeded: bool) -> None:
        """The bridge keys into an evaluation-key dict. Slot 0 alone: bridge_key
        (bridge_mask_key / bridge_key_body), as ever. Further slots (§8.17):
        bridge_keys [G, words] (bridge_mask_keys [G, 8] / bridge_key_bodies
        [G, words]), the occupied slots in ascending order, and their one
        bridge_gadget."""
        slots = self.bridge_slots()
        if not slots:
            return
        gadgets = {self.bridge_gadget_of(s) for s in slots}
        if len(gadgets) != 1:
            raise ValueError(f"the bridge slots hold different gadgets {sorted(gadgets)}: one dict carries one")
        out["bridge_gadget"] = np.array(gadgets.pop(), dtype=np.int64)
        if slots == [0]:
            if seeded:
                out["bridge_mask_key"], out["bridge_key_body"] = self.export_bridge_key_seeded()
            else:
                out["bridge_key"] = self.export_bridge_key()
        elif seeded:
            pairs = [self.export_bridge_key_seeded(s) for s in slots]
            out["bridge_mask_keys"] = np.stack([mk for mk, _ in pairs])
            out["bridge_key_bodies"] = np.stack([body for _, body in pairs])
        else:
            out["bridge_keys"] = np.stack([self.export_bridge_key(s) for s in slots])

    def _import_bridges(self, d: dict) -> None:
        """The multi-bridge entries of a dict (§8.17): row g into slot g;
        every slot from G on is dropped."""
        if "bridge_keys" not in d and "bridge_key_bodies" not in d:
            return
        b, L = (int(x) for x in np.asarray(d["bridge_gadget"]).reshape(2))
        if "bridge_keys" in d:
            rows = np.asarray(d["bridge_keys"])
            rows = rows.reshape(-1, self.bridge_key_words(b, L))
            if not 1 <= len(rows) <= _lib.BRIDGE_SLOTS:
                raise ValueError(f"bridge_keys holds {len(rows)} keys, a context 1 to {_lib.BRIDGE_SLOTS}")
            for g, row in enumerate(rows):
                self.import_bridge_key(b, L, row, slot=g)
        else:
            masks = np.asarray(d["bridge_mask_keys"]).reshape(-1, 8)
            rows = np.asarray(d["bridge_key_bodies"]).reshape(len(masks), -1)
            if not 1 <= len(rows) <= _lib.BRIDGE_SLOTS:
                raise ValueError(f"bridge_key_bodies holds {len(rows)} keys, a context 1 to {_lib.BRIDGE_SLOTS}")
            for g, (mk, row) in enumerate(zip(masks, rows)):
                self.import_bridge_key_seeded(b, L, mk, row, slot=g)
        for s in [s for s in self.bridge_slots() if s >= len(rows)]:
            self.drop_bridge_key(s)

    def export_eval_keys(self, seeded: bool = False) -> dict:
        """Everything a server needs and nothing more, as numpy arrays: bsk,
        ksk, every present gadget's key (gadget_bsk1..5) and, when one was
        generated, the packing key with its gadget (pack_key, pack_gadget) and
        the bridge key with its (bridge_key, bridge_gadget). seeded=True: the
        seeded form of §8.16 instead (eval_mask_key, bsk_body, ksk_body,
        gadget_bsk{g}_body, pack_mask_key / pack_key_body, bridge_mask_key /
        bridge_key_body, the gadgets as before), a third of the bytes or less;
        every key must have been generated or imported seeded."""
        if seeded:
            return self._export_eval_keys_seeded()
        from .params import gadget_level
        p = self.params
        out = {"bsk": np.zeros(self._L.fhe_bsk_words(C.byref(self._P)), np.uint64),
               "ksk": np.zeros(self._L.fhe_ksk_words(C.byref(self._P)), np.uint64)}
        self._chk(self._L.fhe_export_keys(self._ctx, None, None, C.c_void_p(out["bsk"].ctypes.data),
                                          C.c_void_p(out["ksk"].ctypes.data)))
        for g in (1, 2, 3, 4, 5):
            if gadget_level(p, g):
                out[f"gadget_bsk{g}"] = self.export_fast_bsk(g)
        if self.pack_gadget:
            out["pack_key"] = self.export_pack_key()
            out["pack_gadget"] = np.array(self.pack_gadget, dtype=np.int64)
        self._export_bridges(out, False)
        return out

    def _import_eval_keys_seeded(self, d: dict) -> None:
        sizes = seeded_eval_key_sizes(self.params, d)          # ValueError on a size that does not match
        arr = {k: np.ascontiguousarray(d[k], dtype=np.uint64) for k in sizes}
        ptrs = (C.c_void_p * 5)(*[arr[f"gadget_bsk{g}_body"].ctypes.data if f"gadget_bsk{g}_body" in arr else None
                                  for g in (1, 2, 3, 4, 5)])
        self._chk(self._L.fhe_import_eval_keys_seeded(self._ctx, self._key(d["eval_mask_key"]),
                                                      C.c_void_p(arr["bsk_body"].ctypes.data),
                                                      C.c_void_p(arr["ksk_body"].ctypes.data), ptrs))
        self.has_keys = True
        if "pack_key_body" in d:
            b, L = (int(x) for x in np.asarray(d["pack_gadget"]).reshape(2))
            self.import_pack_key_seeded(b, L, d["pack_mask_key"], arr["pack_key_body"])
        if "bridge_key_body" in d:
            b, L = (int(x) for x in np.asarray(d["bridge_gadget"]).reshape(2))
            self.import_bridge_key_seeded(b, L, d["bridge_mask_key"], arr["bridge_key_body"])
        self._import_bridges(d)

    def import_eval_keys(self, d: dict) -> None:
        """Install evaluation keys only (fhe_import_eval_keys; the packing key
        too when the dict has one). The context holds no secret key afterwards.
        A seeded dict (export_eval_keys(seeded=True)) goes through
        fhe_import_eval_keys_seeded; a dict that holds both forms is refused."""
        if eval_keys_seeded(d):
            return self._import_eval_keys_seeded(d)
        bsk = np.ascontiguousarray(d["bsk"], dtype=np.uint64)
        ksk = np.ascontiguousarray(d["ksk"], dtype=np.uint64)
        if bsk.size != self._L.fhe_bsk_words(C.byref(self._P)) or ksk.size != self._L.fhe_ksk_words(C.byref(self._P)):
            raise ValueError("evaluation keys do not match these parameters")
        gad = [np.ascontiguousarray(d[f"gadget_bsk{g}"], dtype=np.uint64) if f"gadget_bsk{g}" in d else None
               for g in (1, 2, 3, 4, 5)]
        for g, a in enumerate(gad, 1):
            if a is not None and a.size != self._L.fhe_fast_bsk_words(C.byref(self._P), g):
                raise ValueError(f"gadget {g}'s key does not match these parameters")
        ptrs = (C.c_void_p * 5)(*[a.ctypes.data if a is not None else None for a in gad])
        self._chk(self._L.fhe_import_eval_keys(self._ctx, C.c_void_p(bsk.ctypes.data), C.c_void_p(ksk.ctypes.data),
                                               ptrs))
        self.has_keys = True
        if "pack_key" in d:
            b, L = (int(x) for x in np.asarray(d["pack_gadget"]).reshape(2))
            self.import_pack_key(b, L, d["pack_key"])
        if "bridge_key" in d:
            b, L = (int(x) for x in np.asarray(d["bridge_gadget"]).reshape(2))
            self.import_bridge_key(b, L, d["bridge_key"])
        self._import_bridges(d)

    def glwe_count(self, count: int) -> int:
        return -(-int(count) // self.params.N)

    def pack(self, ct: torch.Tensor, count: int, levels: int = 0) -> torch.Tensor:
        """count big LWEs -> ceil(count / N) GLWEs of (k+1)N words (fhe_pack_batch)."""
        out = torch.empty((self.glwe_count(count), (self.params.k + 1) * self.params.N), dtype=torch.int64,
                          device=self.device)
        self._chk(self._L.fhe_pack_batch(self._ctx, _ptr(ct), int(count), int(levels), _ptr(out),
                                         _stream(self.device)))
        return out

    def decrypt_packed(self, glwe: torch.Tensor, count: int, mode: int = 0) -> torch.Tensor:
        """The first count coefficients of packed GLWEs (fhe_decrypt_packed_batch):
        mode 0 signed values, 1 bits, 2 raw phases."""
        out = torch.empty(int(count), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_decrypt_packed_batch(self._ctx, _ptr(glwe), int(count), int(mode), _ptr(out),
                                                   _stream(self.device)))
        return out

    def search_query(self, qbody: torch.Tensor, id0: int, mask_key, docs8: torch.Tensor, B: int, D: int,
                     w: torch.Tensor, cst: int, T: int, levels_bit: int = 0):
        """fhe_search_query_batch: the server side of the two-party private
        query; (glwe_acc, glwe_bit), each ceil(B / N) x (k+1)N words."""
        shape = (self.glwe_count(B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_query_batch(self._ctx, _ptr(qbody), C.c_uint64(int(id0)), self._key(mask_key),
                                                 _ptr(docs8), int(B), int(D), _ptr(w), int(cst), int(T),
                                                 int(levels_bit), _ptr(ga), _ptr(gb), _stream(self.device)))
        return ga, gb

    # --------------- several queries of one key holder in one pass (§8.8) --
    @staticmethod
    def _i64s(vals):
        a = np.ascontiguousarray([int(v) for v in vals], dtype=np.int64)
        return a, C.c_void_p(a.ctypes.data)

    def linear_queries(self, ct_q: torch.Tensor, Q: int, docs8: torch.Tensor, B: int, D: int, w, csts,
                       out: torch.Tensor | None = None) -> torch.Tensor:
        """fhe_linear_queries_batch: ct_q Q * D x (kN+1), csts Q host
        constants; Q * B x (kN+1), query-major."""
        wd = self.to_dev(w)
        if out is None:
            out = self.empty_big(Q * B)
        keep, hc = self._i64s(csts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} constants for {Q} queries")
        self._chk(self._L.fhe_linear_queries_batch(self._ctx, _ptr(ct_q), int(Q), _ptr(docs8), int(B), int(D),
                                                   _ptr(wd), hc, _ptr(out), _stream(self.device)))
        return out

    def compare_queries(self, qbody: torch.Tensor, id0: torch.Tensor, mask_key, docs8: torch.Tensor, B: int, D: int,
                        w: torch.Tensor, cst: int, Ts):
        """fhe_compare_queries_batch: Q seeded queries (qbody [Q, D], id0 [Q],
        both on the device) against packed clear documents;
        (acc int64 [Q, B], below int64 [Q, B])."""
        keep, hT = self._i64s(Ts)
        Q = keep.size
        acc = torch.empty((Q, B), dtype=torch.int64, device=self.device)
        below = torch.empty((Q, B), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_compare_queries_batch(self._ctx, _ptr(qbody), _ptr(id0), self._key(mask_key), Q,
                                                    _ptr(docs8), int(B), int(D), _ptr(w), int(cst), hT, _ptr(acc),
                                                    _ptr(below), _stream(self.device)))
        return acc, below

    def search_queries(self, qbody: torch.Tensor, id0: torch.Tensor, mask_key, docs8: torch.Tensor, B: int, D: int,
                       w: torch.Tensor, cst: int, Ts, levels_bit: int = 0):
        """fhe_search_queries_batch: the evaluation-only form;
        (glwe_acc, glwe_bit), each ceil(Q B / N) x (k+1)N words."""
        keep, hT = self._i64s(Ts)
        Q = keep.size
        shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_queries_batch(self._ctx, _ptr(qbody), _ptr(id0), self._key(mask_key), Q,
                                                   _ptr(docs8), int(B), int(D), _ptr(w), int(cst), hT,
                                                   int(levels_bit), _ptr(ga), _ptr(gb), _stream(self.device)))
        return ga, gb

    # --------- stored-ciphertext search: several clear queries in one pass (§8.9) --
    def linear_seeded_queries(self, body: torch.Tensor, id0: torch.Tensor, mask_key, W, csts,
                              out: torch.Tensor | None = None) -> torch.Tensor:
        """fhe_linear_seeded_queries_batch: body [B, D], id0 [B], W int64
        [Q, D], csts Q host constants; Q * B x (kN+1), query-major."""
        B, D = body.shape
        Wd = self.to_dev(W).reshape(-1, D).contiguous()
        Q = Wd.shape[0]
        keep, hc = self._i64s(csts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} constants for {Q} queries")
        if out is None:
            out = self.empty_big(Q * B)
        self._chk(self._L.fhe_linear_seeded_queries_batch(self._ctx, _ptr(body), _ptr(id0), int(B), int(D),
                                                          self._key(mask_key), int(Q), _ptr(Wd), hc, _ptr(out),
                                                          _stream(self.device)))
        return out

    def compare_seeded_queries(self, body: torch.Tensor, id0: torch.Tensor, mask_key, W: torch.Tensor, cst: int, Ts):
        """fhe_compare_seeded_queries_batch: W int64 [Q, D] (device), Ts Q host
        thresholds; (acc int64 [Q, B], below int64 [Q, B])."""
        B, D = body.shape
        keep, hT = self._i64s(Ts)
        Q = keep.size
        if tuple(W.shape) != (Q, D):
            raise ValueError(f"weights {tuple(W.shape)} for {Q} thresholds of {D} features")
        acc = torch.empty((Q, B), dtype=torch.int64, device=self.device)
        below = torch.empty((Q, B), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_compare_seeded_queries_batch(self._ctx, _ptr(body), _ptr(id0), int(B), int(D),
                                                           self._key(mask_key), Q, _ptr(W), int(cst), hT, _ptr(acc),
                                                           _ptr(below), _stream(self.device)))
        return acc, below

    def search_seeded_queries(self, body: torch.Tensor, id0: torch.Tensor, mask_key, W: torch.Tensor, cst: int, Ts,
                              levels_bit: int = 0, b_old: int = 0):
        """fhe_search_seeded_queries_batch: the evaluation-only form;
        (glwe_acc, glwe_bit), each ceil(Q B / N) x (k+1)N words. b_old > 0:
        the first b_old documents are under a rotated-out key and go through
        the bridge key (fhe_search_seeded_queries_bridged_batch, §8.12)."""
        B, D = body.shape
        if b_old:
            keep, hT = self._i64s(Ts)
            Q = keep.size
            if tuple(W.shape) != (Q, D):
                raise ValueError(f"weights {tuple(W.shape)} for {Q} thresholds of {D} features")
            shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
            ga = torch.empty(shape, dtype=torch.int64, device=self.device)
            gb = torch.empty(shape, dtype=torch.int64, device=self.device)
            self._chk(self._L.fhe_search_seeded_queries_bridged_batch(
                self._ctx, _ptr(body), _ptr(id0), int(B), int(D), self._key(mask_key), Q, _ptr(W), int(cst), hT,
                int(levels_bit), int(b_old), _ptr(ga), _ptr(gb), _stream(self.device)))
            return ga, gb
        keep, hT = self._i64s(Ts)
        Q = keep.size
        if tuple(W.shape) != (Q, D):
            raise ValueError(f"weights {tuple(W.shape)} for {Q} thresholds of {D} features")
        shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_seeded_queries_batch(self._ctx, _ptr(body), _ptr(id0), int(B), int(D),
                                                          self._key(mask_key), Q, _ptr(W), int(cst), hT,
                                                          int(levels_bit), _ptr(ga), _ptr(gb), _stream(self.device)))
        return ga, gb

    def search_seeded_queries_gens(self, body: torch.Tensor, id0: torch.Tensor, mask_key, W: torch.Tensor, cst: int,
                                   Ts, levels_bit: int = 0, gen_ends=(), gen_slots=()):
        """fhe_search_seeded_queries_gens_batch: search_seeded_queries with
        several old generations resident (§8.17): documents gen_ends[g - 1] <=
        b < gen_ends[g] go through bridge slot gen_slots[g], the documents
        after gen_ends[-1] are under the current key."""
        B, D = body.shape
        keep, hT = self._i64s(Ts)
        Q = keep.size
        if tuple(W.shape) != (Q, D):
            raise ValueError(f"weights {tuple(W.shape)} for {Q} thresholds of {D} features")
        G, he, hs = self._gens(gen_ends, gen_slots)
        shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_seeded_queries_gens_batch(
            self._ctx, _ptr(body), _ptr(id0), int(B), int(D), self._key(mask_key), Q, _ptr(W), int(cst), hT,
            int(levels_bit), G, he, hs, _ptr(ga), _ptr(gb), _stream(self.device)))
        return ga, gb

    # ------------- both-private search: GGSW query x GLWE documents (§8.7) --
    def ggsw_words(self, base_log: int, level: int) -> int:
        return self._L.fhe_ggsw_words(C.byref(self._P), int(base_log), int(level))

    def doc_slots(self, D: int) -> int:
        """Documents of D features per GLWE."""
        if not 0 < D <= self.params.N:
            raise ValueError(f"a document of D = {D} features does not fit one GLWE (N = {self.params.N})")
        return self.params.N // D

    def doc_glwes(self, B: int, D: int) -> int:
        return -(-int(B) // self.doc_slots(D))

    def encrypt_docs_glwe(self, dq, enc, id0: int = 0) -> torch.Tensor:
        """Quantized documents (int64 [B, D]) -> ceil(B / S) GLWEs, S = N // D
        documents each, feature j of document i at coefficient i D + j
        (fhe_encrypt_packed_batch[_key] on rows of S D values). `enc` is an int
        seed (tests) or a 256-bit stream key; GLWE g uses stream id id0 + g."""
        m = self.to_dev(dq)
        B, D = m.shape
        S, G = self.doc_slots(D), self.doc_glwes(B, D)
        rows = torch.zeros((G * S, D), dtype=torch.int64, device=self.device)
        rows[:B] = m
        rows = rows.reshape(G, S * D).contiguous()
        out = torch.empty((G, (self.params.k + 1) * self.params.N), dtype=torch.int64, device=self.device)
        if isinstance(enc, (int, np.integer)):
            rc = self._L.fhe_encrypt_packed_batch(self._ctx, _ptr(rows), G, S * D, C.c_uint64(int(enc)),
                                                  C.c_uint64(id0), _ptr(out), _stream(self.device))
        else:
            rc = self._L.fhe_encrypt_packed_batch_key(self._ctx, _ptr(rows), G, S * D, self._key(enc),
                                                      C.c_uint64(id0), _ptr(out), _stream(self.device))
        self._chk(rc)
        return out

    def encrypt_ggsw(self, w, base_log: int, level: int, enc, id0: int = 0) -> torch.Tensor:
        """GGSW of Q = sum_j w[j] X^-j (fhe_encrypt_ggsw[_key]): int64
        [(k+1) level, k+1, N] words. `enc` as in encrypt_docs_glwe."""
        wd = self.to_dev(np.asarray(w, dtype=np.int64) if not isinstance(w, torch.Tensor) else w).reshape(-1)
        p = self.params
        out = torch.empty(((p.k + 1) * int(level), p.k + 1, p.N), dtype=torch.int64, device=self.device)
        if isinstance(enc, (int, np.integer)):
            rc = self._L.fhe_encrypt_ggsw(self._ctx, _ptr(wd), wd.numel(), int(base_log), int(level),
                                          C.c_uint64(int(enc)), C.c_uint64(id0), _ptr(out), _stream(self.device))
        else:
            rc = self._L.fhe_encrypt_ggsw_key(self._ctx, _ptr(wd), wd.numel(), int(base_log), int(level),
                                              self._key(enc), C.c_uint64(id0), _ptr(out), _stream(self.device))
        self._chk(rc)
        return out

    def pack_docs_glwe(self, glwe: torch.Tensor, B: int, D: int, base_log: int, level: int) -> torch.Tensor:
        """Document GLWEs -> the i8 digit operand of linear_ggsw / compare_ggsw
        / search_ggsw (fhe_glwe_docs_pack), once per resident corpus."""
        n = self._L.fhe_glwe_docs_bytes(C.byref(self._P), int(B), int(D), int(level))
        docs8 = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._chk(self._L.fhe_glwe_docs_pack(self._ctx, _ptr(glwe), int(B), int(D), int(base_log), int(level),
                                             _ptr(docs8), _stream(self.device)))
        return docs8

    def linear_ggsw(self, ggsw: torch.Tensor, base_log: int, level: int, docs8: torch.Tensor, B: int, D: int,
                    cst: int) -> torch.Tensor:
        """The exact external product and slot extraction (fhe_linear_ggsw_batch): B x (kN+1)."""
        out = self.empty_big(B)
        self._chk(self._L.fhe_linear_ggsw_batch(self._ctx, _ptr(ggsw), int(base_log), int(level), _ptr(docs8), int(B),
                                                int(D), int(cst), _ptr(out), _stream(self.device)))
        return out

    def compare_ggsw(self, ggsw: torch.Tensor, base_log: int, level: int, docs8: torch.Tensor, B: int, D: int,
                     cst: int, T: int):
        """fhe_compare_ggsw_batch: (acc int64[B], below int64[B])."""
        acc = torch.empty(B, dtype=torch.int64, device=self.device)
        below = torch.empty(B, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_compare_ggsw_batch(self._ctx, _ptr(ggsw), int(base_log), int(level), _ptr(docs8), int(B),
                                                 int(D), int(cst), int(T), _ptr(acc), _ptr(below),
                                                 _stream(self.device)))
        return acc, below

    def search_ggsw(self, ggsw: torch.Tensor, base_log: int, level: int, docs8: torch.Tensor, B: int, D: int,
                    cst: int, T: int, levels_bit: int = 0):
        """fhe_search_ggsw_batch: the untrusted host's entry; (glwe_acc,
        glwe_bit), each ceil(B / N) x (k+1)N words."""
        shape = (self.glwe_count(B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_ggsw_batch(self._ctx, _ptr(ggsw), int(base_log), int(level), _ptr(docs8), int(B),
                                                int(D), int(cst), int(T), int(levels_bit), _ptr(ga), _ptr(gb),
                                                _stream(self.device)))
        return ga, gb

    # ------------- both-private search: several GGSW queries in one pass (§8.10) --
    def ggsws_ws_bytes(self, Q: int, B: int, D: int, level: int) -> int:
        """Context workspace of a batched call (fhe_ggsws_ws_bytes; host only)."""
        return self._L.fhe_ggsws_ws_bytes(C.byref(self._P), int(Q), int(B), int(D), int(level))

    def pack_docs_glwe_queries(self, glwe: torch.Tensor, B: int, D: int, base_log: int, level: int) -> torch.Tensor:
        """Document GLWEs -> the resident operand of linear_ggsws /
        compare_ggsws / search_ggsws (fhe_glwe_docs_queries_pack)."""
        n = self._L.fhe_glwe_docs_queries_bytes(C.byref(self._P), int(B), int(D), int(level))
        docs = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._chk(self._L.fhe_glwe_docs_queries_pack(self._ctx, _ptr(glwe), int(B), int(D), int(base_log), int(level),
                                                     _ptr(docs), _stream(self.device)))
        return docs

    def _ggsws(self, ggsws: torch.Tensor, base_log: int, level: int) -> int:
        words = self.ggsw_words(base_log, level)
        if words == 0 or ggsws.numel() == 0 or ggsws.numel() % words:
            raise ValueError(f"{ggsws.numel()} words are no whole number of GGSWs of gadget ({base_log}, {level})")
        return ggsws.numel() // words

    def linear_ggsws(self, ggsws: torch.Tensor, base_log: int, level: int, docs: torch.Tensor, B: int, D: int, csts,
                     out: torch.Tensor | None = None) -> torch.Tensor:
        """fhe_linear_ggsws_batch: ggsws Q x ggsw_words (device), csts Q host
        constants; Q * B x (kN+1), query-major."""
        Q = self._ggsws(ggsws, base_log, level)
        keep, hc = self._i64s(csts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} constants for {Q} queries")
        if out is None:
            out = self.empty_big(Q * B)
        self._chk(self._L.fhe_linear_ggsws_batch(self._ctx, _ptr(ggsws), int(base_log), int(level), _ptr(docs), Q,
                                                 int(B), int(D), hc, _ptr(out), _stream(self.device)))
        return out

    def compare_ggsws(self, ggsws: torch.Tensor, base_log: int, level: int, docs: torch.Tensor, B: int, D: int,
                      cst: int, Ts):
        """fhe_compare_ggsws_batch: Ts Q host thresholds;
        (acc int64 [Q, B], below int64 [Q, B])."""
        Q = self._ggsws(ggsws, base_log, level)
        keep, hT = self._i64s(Ts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} thresholds for {Q} queries")
        acc = torch.empty((Q, B), dtype=torch.int64, device=self.device)
        below = torch.empty((Q, B), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_compare_ggsws_batch(self._ctx, _ptr(ggsws), int(base_log), int(level), _ptr(docs), Q,
                                                  int(B), int(D), int(cst), hT, _ptr(acc), _ptr(below),
                                                  _stream(self.device)))
        return acc, below

    def search_ggsws(self, ggsws: torch.Tensor, base_log: int, level: int, docs: torch.Tensor, B: int, D: int,
                     cst: int, Ts, levels_bit: int = 0):
        """fhe_search_ggsws_batch: the evaluation-only form;
        (glwe_acc, glwe_bit), each ceil(Q B / N) x (k+1)N words."""
        Q = self._ggsws(ggsws, base_log, level)
        keep, hT = self._i64s(Ts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} thresholds for {Q} queries")
        shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_ggsws_batch(self._ctx, _ptr(ggsws), int(base_log), int(level), _ptr(docs), Q,
                                                 int(B), int(D), int(cst), hT, int(levels_bit), _ptr(ga), _ptr(gb),
                                                 _stream(self.device)))
        return ga, gb

    # ---- both-private key rotation: per-generation GGSW queries (§8.19) --
    def ggsws_gens_ws_bytes(self, Q: int, Bs, D: int, level: int) -> int:
        """Product workspace of a generations call (fhe_ggsws_gens_ws_bytes; host only)."""
        keep, hB = self._i64s(Bs)
        return self._L.fhe_ggsws_gens_ws_bytes(C.byref(self._P), int(Q), hB, keep.size, int(D), int(level))

    def _ggsw_gens(self, gens, base_log: int, level: int):
        """gens: (slot, ggsws, docs, B) per generation, oldest first; ggsws and
        docs may be None where B == 0. -> (the fhe_ggsw_gen array, Q, B)."""
        arr = (_lib.FheGgswGen * max(1, len(gens)))()
        Q = None
        for i, (slot, ggsws, docs, B) in enumerate(gens):
            if int(B) > 0:
                q = self._ggsws(ggsws, base_log, level)
                if Q is not None and q != Q:
                    raise ValueError(f"generation {i} holds {q} queries, an earlier one {Q}")
                Q = q
            a = arr[i]
            a.struct_size, a.slot, a.B = C.sizeof(_lib.FheGgswGen), int(slot), int(B)
            if int(B) > 0:
                assert ggsws.is_contiguous() and docs.is_contiguous(), "buffers must be contiguous"
                a.d_ggsw, a.d_docs = ggsws.data_ptr(), docs.data_ptr()
        if Q is None:
            raise ValueError("no generation holds a document")
        return arr, Q, sum(int(g[3]) for g in gens)

    def linear_ggsws_gens(self, gens, base_log: int, level: int, D: int, csts,
                          out: torch.Tensor | None = None) -> torch.Tensor:
        """fhe_linear_ggsws_gens_batch: gens (slot, ggsws, docs, B) per key
        generation, oldest first; Q * B x (kN+1), query-major, generation g's
        documents from off_g on, each row under its own generation's key."""
        arr, Q, B = self._ggsw_gens(gens, base_log, level)
        keep, hc = self._i64s(csts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} constants for {Q} queries")
        if out is None:
            out = self.empty_big(Q * B)
        self._chk(self._L.fhe_linear_ggsws_gens_batch(self._ctx, C.byref(arr), len(gens), int(base_log), int(level), Q,
                                                      int(D), hc, _ptr(out), _stream(self.device)))
        return out

    def search_ggsws_gens(self, gens, base_log: int, level: int, D: int, cst: int, Ts, levels_bit: int = 0):
        """fhe_search_ggsws_gens_batch: the evaluation-only form over several
        key generations, the old ones' rows bridged to the current key;
        (glwe_acc, glwe_bit), each ceil(Q B / N) x (k+1)N words, B = sum B_g."""
        arr, Q, B = self._ggsw_gens(gens, base_log, level)
        keep, hT = self._i64s(Ts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} thresholds for {Q} queries")
        shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_ggsws_gens_batch(self._ctx, C.byref(arr), len(gens), int(base_log), int(level), Q,
                                                      int(D), int(cst), hT, int(levels_bit), _ptr(ga), _ptr(gb),
                                                      _stream(self.device)))
        return ga, gb

    # ------- both-private search on seeded documents and queries (§8.15) --
    def ggsw_body_words(self, base_log: int, level: int) -> int:
        return self._L.fhe_ggsw_body_words(C.byref(self._P), int(base_log), int(level))

    def _ids(self, id0s) -> torch.Tensor:
        """Stream ids (python ints modulo 2^64) as a device int64 tensor."""
        a = np.array([int(i) % (1 << 64) for i in id0s], dtype=np.uint64)
        return torch.from_numpy(a.view(np.int64)).to(self.device)

    def encrypt_docs_glwe_seeded(self, dq, mask_key, noise_key, id0: int = 0) -> torch.Tensor:
        """encrypt_docs_glwe with a public mask key and a secret noise key:
        the bodies alone, int64 [G, N] (fhe_encrypt_packed_seeded_batch)."""
        m = self.to_dev(dq)
        B, D = m.shape
        S, G = self.doc_slots(D), self.doc_glwes(B, D)
        rows = torch.zeros((G * S, D), dtype=torch.int64, device=self.device)
        rows[:B] = m
        rows = rows.reshape(G, S * D).contiguous()
        out = torch.empty((G, self.params.N), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_encrypt_packed_seeded_batch(self._ctx, _ptr(rows), G, S * D, self._key(mask_key),
                                                          self._key(noise_key), C.c_uint64(int(id0) % (1 << 64)),
                                                          _ptr(out), _stream(self.device)))
        return out

    def encrypt_ggsw_seeded(self, w, base_log: int, level: int, mask_key, noise_key, id0: int = 0) -> torch.Tensor:
        """encrypt_ggsw's bodies alone, int64 [(k+1) level, N] (fhe_encrypt_ggsw_seeded)."""
        wd = self.to_dev(np.asarray(w, dtype=np.int64) if not isinstance(w, torch.Tensor) else w).reshape(-1)
        p = self.params
        out = torch.empty(((p.k + 1) * int(level), p.N), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_encrypt_ggsw_seeded(self._ctx, _ptr(wd), wd.numel(), int(base_log), int(level),
                                                  self._key(mask_key), self._key(noise_key),
                                                  C.c_uint64(int(id0) % (1 << 64)), _ptr(out), _stream(self.device)))
        return out

    def expand_docs_glwe_seeded(self, body: torch.Tensor, id0: int, mask_key) -> torch.Tensor:
        """Seeded document bodies [G, N] -> full-form GLWEs [G, (k+1)N] (fhe_expand_packed_seeded_batch)."""
        p = self.params
        G = body.numel() // p.N
        out = torch.empty((G, (p.k + 1) * p.N), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_expand_packed_seeded_batch(self._ctx, _ptr(body), C.c_uint64(int(id0) % (1 << 64)), G,
                                                         p.N, self._key(mask_key), _ptr(out), _stream(self.device)))
        return out

    def expand_ggsws_seeded(self, bodies: torch.Tensor, id0s, base_log: int, level: int, mask_key) -> torch.Tensor:
        """Q seeded queries' bodies -> Q full-form GGSWs, int64 [Q, ggsw_words] (fhe_expand_ggsws_seeded)."""
        ids = self._ids(id0s)
        Q = ids.numel()
        bw = self.ggsw_body_words(base_log, level)
        if bw == 0 or bodies.numel() != Q * bw:
            raise ValueError(f"{bodies.numel()} words are not the bodies of {Q} GGSWs of gadget ({base_log}, {level})")
        out = torch.empty((Q, self.ggsw_words(base_log, level)), dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_expand_ggsws_seeded(self._ctx, _ptr(bodies), _ptr(ids), Q, int(base_log), int(level),
                                                  self._key(mask_key), _ptr(out), _stream(self.device)))
        return out

    def pack_docs_glwe_seeded(self, body: torch.Tensor, id0: int, mask_key, B: int, D: int, base_log: int,
                              level: int, queries: bool = False) -> torch.Tensor:
        """pack_docs_glwe (queries=True: pack_docs_glwe_queries) straight from
        seeded bodies: the same operand byte for byte, the masks regenerated
        in registers (fhe_glwe_docs_pack_seeded, fhe_glwe_docs_queries_pack_seeded)."""
        size = self._L.fhe_glwe_docs_queries_bytes if queries else self._L.fhe_glwe_docs_bytes
        pack = self._L.fhe_glwe_docs_queries_pack_seeded if queries else self._L.fhe_glwe_docs_pack_seeded
        if body.numel() != self.doc_glwes(B, D) * self.params.N:
            raise ValueError(f"{body.numel()} body words for {self.doc_glwes(B, D)} document GLWEs")
        docs = torch.empty(size(C.byref(self._P), int(B), int(D), int(level)), dtype=torch.uint8, device=self.device)
        self._chk(pack(self._ctx, _ptr(body), C.c_uint64(int(id0) % (1 << 64)), int(B), int(D), int(base_log),
                       int(level), self._key(mask_key), _ptr(docs), _stream(self.device)))
        return docs

    def search_ggsw_seeded(self, body: torch.Tensor, id0: int, mask_key, base_log: int, level: int,
                           docs8: torch.Tensor, B: int, D: int, cst: int, T: int, levels_bit: int = 0):
        """search_ggsw on one seeded query (fhe_search_ggsw_seeded_batch)."""
        shape = (self.glwe_count(B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_ggsw_seeded_batch(self._ctx, _ptr(body), C.c_uint64(int(id0) % (1 << 64)),
                                                       int(base_log), int(level), self._key(mask_key), _ptr(docs8),
                                                       int(B), int(D), int(cst), int(T), int(levels_bit), _ptr(ga),
                                                       _ptr(gb), _stream(self.device)))
        return ga, gb

    def search_ggsws_seeded(self, bodies: torch.Tensor, id0s, mask_key, base_log: int, level: int,
                            docs: torch.Tensor, B: int, D: int, cst: int, Ts, levels_bit: int = 0):
        """search_ggsws on Q seeded queries (fhe_search_ggsws_seeded_batch)."""
        ids = self._ids(id0s)
        Q = ids.numel()
        keep, hT = self._i64s(Ts)
        if keep.size != Q:
            raise ValueError(f"{keep.size} thresholds for {Q} queries")
        if bodies.numel() != Q * self.ggsw_body_words(base_log, level):
            raise ValueError(f"{bodies.numel()} words are not the bodies of {Q} GGSWs of gadget ({base_log}, {level})")
        shape = (self.glwe_count(Q * B), (self.params.k + 1) * self.params.N)
        ga = torch.empty(shape, dtype=torch.int64, device=self.device)
        gb = torch.empty(shape, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_search_ggsws_seeded_batch(self._ctx, _ptr(bodies), _ptr(ids), int(base_log), int(level),
                                                        self._key(mask_key), _ptr(docs), Q, int(B), int(D), int(cst),
                                                        hT, int(levels_bit), _ptr(ga), _ptr(gb),
                                                        _stream(self.device)))
        return ga, gb

    def topk(self, acc: torch.Tensor, below: torch.Tensor | None, k: int, base_idx: int = 0):
        oa = torch.empty(k, dtype=torch.int64, device=self.device)
        oi = torch.empty(k, dtype=torch.int64, device=self.device)
        self._chk(self._L.fhe_topk(self._ctx, _ptr(acc), _ptr(below), acc.numel(), base_idx, k, _ptr(oa), _ptr(oi),
                                   _stream(self.device)))
        return oa, oi

    # --------------------------------------------------------- measurement --
    def profile(self, enable: bool) -> None:
        self._chk(self._L.fhe_profile_enable(self._ctx, int(enable)))

    def kernel_name(self, kernel: str) -> str:
        """The instantiation last launched for a profile bucket (fhe_profile_kernel_name)."""
        buf = C.create_string_buffer(256)
        self._chk(self._L.fhe_profile_kernel_name(self._ctx, kernel.encode(), buf, 256))
        return buf.value.decode()

    def profile_read(self, kernel: str) -> dict:
        ms = C.c_double()
        nl = C.c_int64()
        items = C.c_int64()
        self._chk(self._L.fhe_profile_read(self._ctx, kernel.encode(), C.byref(ms), C.byref(nl), C.byref(items)))
        return {"total_ms": ms.value, "launches": nl.value, "items": items.value}


FULL_EVAL_KEYS = ("bsk", "ksk", "pack_key", "bridge_key", "bridge_keys") + \
    tuple(f"gadget_bsk{g}" for g in (1, 2, 3, 4, 5))


def eval_keys_seeded(d: dict) -> bool:
    """Which form an evaluation-key dict has: True for the seeded form of
    DESIGN.md §8.16 (it has "bsk_body"), False for the full form. A dict with
    arrays of both forms is a ValueError."""
    seeded = "bsk_body" in d
    if seeded:
        both = [k for k in FULL_EVAL_KEYS if k in d]
        if both:
            raise ValueError(f"evaluation keys mix the seeded and the full form: bsk_body and {', '.join(both)}")
        for k in ("eval_mask_key", "ksk_body"):
            if k not in d:
                raise ValueError(f"seeded evaluation keys without {k}")
    elif any(k.endswith("_body") or k == "bridge_key_bodies" for k in d):
        raise ValueError("evaluation keys mix the seeded and the full form: bodies without bsk_body")
    return seeded


def seeded_eval_key_sizes(params: SchemeParams, d: dict) -> dict:
    """name -> words of every body array a seeded dict must and does hold for
    these parameters (the ABI's size functions); ValueError naming the array
    whose size differs, a missing gadget's key or a mask key that is not 8 words."""
    from .params import gadget_level
    L = _lib.lib()
    P = _lib.params_struct(params.as_dict())
    want = {"bsk_body": L.fhe_bsk_body_words(C.byref(P)), "ksk_body": L.fhe_ksk_body_words(C.byref(P))}
    for g in (1, 2, 3, 4, 5):
        if gadget_level(params, g):
            want[f"gadget_bsk{g}_body"] = L.fhe_fast_bsk_body_words(C.byref(P), g)
    masks = ["eval_mask_key"]
    for name, fn in (("pack", L.fhe_pack_key_body_words), ("bridge", L.fhe_bridge_key_body_words)):
        if f"{name}_key_body" in d:
            if f"{name}_gadget" not in d or f"{name}_mask_key" not in d:
                raise ValueError(f"{name}_key_body without {name}_gadget or {name}_mask_key")
            b, lv = (int(x) for x in np.asarray(d[f"{name}_gadget"]).reshape(2))
            want[f"{name}_key_body"] = fn(C.byref(P), b, lv)
            masks.append(f"{name}_mask_key")
    if "bridge_key_bodies" in d:
        if "bridge_gadget" not in d or "bridge_mask_keys" not in d:
            raise ValueError("bridge_key_bodies without bridge_gadget or bridge_mask_keys")
        b, lv = (int(x) for x in np.asarray(d["bridge_gadget"]).reshape(2))
        per = L.fhe_bridge_key_body_words(C.byref(P), b, lv)
        G = np.asarray(d["bridge_mask_keys"]).size // 8
        if per == 0 or np.asarray(d["bridge_mask_keys"]).size != 8 * G or not 1 <= G <= _lib.BRIDGE_SLOTS or \
                np.asarray(d["bridge_key_bodies"]).size != G * per:
            raise ValueError(f"bridge_key_bodies: {np.asarray(d['bridge_key_bodies']).size} words and "
                             f"{np.asarray(d['bridge_mask_keys']).size} mask key words do not match 1 to "
                             f"{_lib.BRIDGE_SLOTS} keys of {per} words")
    for k, n in want.items():
        if k not in d:
            raise ValueError(f"seeded evaluation keys without {k} (these parameters have it)")
        if np.asarray(d[k]).size != n or n == 0:
            raise ValueError(f"{k}: {np.asarray(d[k]).size} words do not match these parameters ({n})")
    for k in masks:
        if np.asarray(d[k]).size != 8:
            raise ValueError(f"{k}: a mask key is 8 words of 32 bits")
    return want


def group_rows(counts) -> tuple:
    """(M, starts) of a group batch (fhe_group_rows): tenant t's counts[t] rows
    start at sum of the earlier tenants' counts, each rounded up to 4."""
    n = len(counts)
    c = (C.c_int64 * max(n, 1))(*[int(x) for x in counts])
    s = (C.c_int64 * max(n, 1))()
    M = _lib.lib().fhe_group_rows(c, n, s)
    if M < 0:
        raise ValueError("group_rows needs counts >= 0")
    return int(M), [int(x) for x in s[:n]]


class EngineGroup:
    """Several key holders in one batched call: engines on
    one device with equal parameters, each with its own evaluation keys. The
    engines are borrowed and must outlive the group."""

    def __init__(self, engines):
        self.engines = list(engines)
        self._L = _lib.lib()
        arr = (C.c_void_p * max(len(self.engines), 1))(*[e._ctx for e in self.engines])
        h = C.c_void_p()
        _lib.check(self._L.fhe_group_create(arr, len(self.engines), C.byref(h)))
        self._grp = h
        self.device = self.engines[0].device
        self.W = self.engines[0].W

    def close(self) -> None:
        if getattr(self, "_grp", None):
            self._L.fhe_group_destroy(self._grp)
            self._grp = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def rows(counts) -> tuple:
        return group_rows(counts)

    def sign(self, ct_v: torch.Tensor, counts) -> torch.Tensor:
        """fhe_sign_group_batch: ct_v holds the M padded rows of rows(counts)
        (consumed); returns M sign rows, the padding rows unwritten."""
        M, _ = group_rows(counts)
        if len(counts) != len(self.engines) or ct_v.numel() != M * self.W:
            raise ValueError(f"{len(counts)} counts and {ct_v.numel() // self.W} rows for {len(self.engines)} tenants "
                             f"and {M} padded rows")
        sign = torch.empty((M, self.W), dtype=torch.int64, device=self.device)
        c = (C.c_int64 * len(counts))(*[int(x) for x in counts])
        _lib.check(self._L.fhe_sign_group_batch(self._grp, _ptr(ct_v), c, _ptr(sign), _stream(self.device)))
        return sign

    def search_queries(self, items) -> list:
        """fhe_search_query_group_batch. items: one per engine, None (the
        tenant sits this call out) or the arguments of Engine.search_queries
        as a tuple (qbody, id0, mask_key, docs8, B, D, w, cst, Ts, levels_bit).
        Returns, per tenant, (glwe_acc, glwe_bit) or None."""
        if len(items) != len(self.engines):
            raise ValueError(f"{len(items)} items for {len(self.engines)} tenants")
        arr = (_lib.FheGroupQuery * len(items))()
        keep, out = [], []
        for t, (eng, it) in enumerate(zip(self.engines, items)):
            arr[t].struct_size = C.sizeof(_lib.FheGroupQuery)
            if it is None:
                out.append(None)
                continue
            qbody, id0, mask_key, docs8, B, D, w, cst, Ts, levels_bit = it
            hT, _ = Engine._i64s(Ts)
            key = Engine._key(mask_key)
            Q = hT.size
            shape = (eng.glwe_count(Q * int(B)), (eng.params.k + 1) * eng.params.N)
            ga = torch.empty(shape, dtype=torch.int64, device=self.device)
            gb = torch.empty(shape, dtype=torch.int64, device=self.device)
            keep.append((hT, key, qbody, id0, docs8, w))
            q = arr[t]
            q.D, q.Q, q.B, q.cst, q.levels_bit = int(D), Q, int(B), int(cst), int(levels_bit)
            q.d_qbody, q.d_id0, q.d_docs8, q.d_w = qbody.data_ptr(), id0.data_ptr(), docs8.data_ptr(), w.data_ptr()
            q.h_mask_key, q.h_T = C.addressof(key), hT.ctypes.data
            q.d_glwe_acc, q.d_glwe_bit = ga.data_ptr(), gb.data_ptr()
            out.append((ga, gb))
        _lib.check(self._L.fhe_search_query_group_batch(self._grp, arr, len(items), _stream(self.device)))
        return out

    def keyswitch(self, big: torch.Tensor, counts, shift: int = 0, add_body: int = 0,
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """fhe_keyswitch_group_batch: big holds the M padded rows of
        rows(counts), kN + 1 words each; returns M small rows (n + 1 words),
        tenant t's under its own key, the padding rows unwritten (`out`: a
        buffer of at least M rows to write into)."""
        M, _ = group_rows(counts)
        if len(counts) != len(self.engines) or big.numel() != M * self.W:
            raise ValueError(f"{len(counts)} counts and {big.numel() // self.W} rows for {len(self.engines)} tenants "
                             f"and {M} padded rows")
        Ws = self.engines[0].params.n + 1
        if out is not None and out.numel() < M * Ws:
            raise ValueError(f"out holds {out.numel() // Ws} rows, the layout {M}")
        small = torch.empty((M, Ws), dtype=torch.int64, device=self.device) if out is None else out
        c = (C.c_int64 * len(counts))(*[int(x) for x in counts])
        _lib.check(self._L.fhe_keyswitch_group_batch(self._grp, _ptr(big), c, int(shift),
                                                     int(add_body) % (1 << 64), _ptr(small), _stream(self.device)))
        return small

    def search_seeded_queries(self, items) -> list:
        """fhe_search_seeded_queries_group_batch. items: one per engine, None
        (the tenant sits this call out) or the arguments of
        Engine.search_seeded_queries as a tuple (body, id0, mask_key, W, cst,
        Ts, levels_bit, b_old). Returns, per tenant, (glwe_acc, glwe_bit) or
        None."""
        if len(items) != len(self.engines):
            raise ValueError(f"{len(items)} items for {len(self.engines)} tenants")
        arr = (_lib.FheGroupCorpus * len(items))()
        keep, out = [], []
        for t, (eng, it) in enumerate(zip(self.engines, items)):
            arr[t].struct_size = C.sizeof(_lib.FheGroupCorpus)
            if it is None:
                out.append(None)
                continue
            body, id0, mask_key, W, cst, Ts, levels_bit, b_old = it
            hT, _ = Engine._i64s(Ts)
            key = Engine._key(mask_key)
            Q = hT.size
            B, D = body.shape
            if tuple(W.shape) != (Q, D):
                raise ValueError(f"tenant {t}: weights {tuple(W.shape)} for {Q} thresholds of {D} features")
            shape = (eng.glwe_count(Q * int(B)), (eng.params.k + 1) * eng.params.N)
            ga = torch.empty(shape, dtype=torch.int64, device=self.device)
            gb = torch.empty(shape, dtype=torch.int64, device=self.device)
            keep.append((hT, key, body, id0, W))
            c = arr[t]
            c.D, c.Q, c.B, c.cst, c.levels_bit, c.B_old = int(D), Q, int(B), int(cst), int(levels_bit), int(b_old)
            c.d_body, c.d_id0, c.d_W = body.data_ptr(), id0.data_ptr(), W.data_ptr()
            c.h_mask_key, c.h_T = C.addressof(key), hT.ctypes.data
            c.d_glwe_acc, c.d_glwe_bit = ga.data_ptr(), gb.data_ptr()
            out.append((ga, gb))
        _lib.check(self._L.fhe_search_seeded_queries_group_batch(self._grp, arr, len(items), _stream(self.device)))
        return out

    # ------------- rotation schedules: one bridge for all tenants (§8.18) --
    def bridge_gens(self, ct: torch.Tensor, maps) -> torch.Tensor:
        """fhe_bridge_group_gens_batch: in place on the padded rows of
        rows([Q_t * B_t]). maps: one per engine, None (the tenant sits this
        call out) or (Q, B, gen_ends, gen_slots) as Engine.bridge_gens."""
        if len(maps) != len(self.engines):
            raise ValueError(f"{len(maps)} row maps for {len(self.engines)} tenants")
        arr = (_lib.FheGroupRowmap * max(len(maps), 1))()
        keep, counts = [], []
        for t, m in enumerate(maps):
            arr[t].struct_size = C.sizeof(_lib.FheGroupRowmap)
            if m is None:
                counts.append(0)
                continue
            Q, B, ends, slots = m
            G, he, hs = Engine._gens(ends, slots)
            keep.append((he, hs))
            arr[t].Q, arr[t].B, arr[t].G = int(Q), int(B), G
            arr[t].h_ends, arr[t].h_slots = C.addressof(he), C.addressof(hs)
            counts.append(int(Q) * int(B))
        M, _ = group_rows(counts)
        if ct.numel() < M * self.W:
            raise ValueError(f"ct holds {ct.numel() // self.W} rows, the layout {M}")
        _lib.check(self._L.fhe_bridge_group_gens_batch(self._grp, _ptr(ct), arr, len(maps), _stream(self.device)))
        return ct

    def search_seeded_queries_gens(self, items) -> list:
        """fhe_search_seeded_queries_group_gens_batch. items: one per engine,
        None (the tenant sits this call out) or search_seeded_queries' tuple
        with (gen_ends, gen_slots) in b_old's place: (body, id0, mask_key, W,
        cst, Ts, levels_bit, gen_ends, gen_slots). Returns, per tenant,
        (glwe_acc, glwe_bit) or None."""
        if len(items) != len(self.engines):
            raise ValueError(f"{len(items)} items for {len(self.engines)} tenants")
        arr = (_lib.FheGroupCorpusGens * max(len(items), 1))()
        keep, out = [], []
        for t, (eng, it) in enumerate(zip(self.engines, items)):
            arr[t].struct_size = C.sizeof(_lib.FheGroupCorpusGens)
            if it is None:
                out.append(None)
                continue
            body, id0, mask_key, W, cst, Ts, levels_bit, ends, slots = it
            hT, _ = Engine._i64s(Ts)
            key = Engine._key(mask_key)
            G, he, hs = Engine._gens(ends, slots)
            Q = hT.size
            B, D = body.shape
            if tuple(W.shape) != (Q, D):
                raise ValueError(f"tenant {t}: weights {tuple(W.shape)} for {Q} thresholds of {D} features")
            shape = (eng.glwe_count(Q * int(B)), (eng.params.k + 1) * eng.params.N)
            ga = torch.empty(shape, dtype=torch.int64, device=self.device)
            gb = torch.empty(shape, dtype=torch.int64, device=self.device)
            keep.append((hT, key, body, id0, W, he, hs))
            c = arr[t]
            c.D, c.Q, c.B, c.cst, c.levels_bit, c.G = int(D), Q, int(B), int(cst), int(levels_bit), G
            c.d_body, c.d_id0, c.d_W = body.data_ptr(), id0.data_ptr(), W.data_ptr()
            c.h_mask_key, c.h_T = C.addressof(key), hT.ctypes.data
            c.h_ends, c.h_slots = C.addressof(he), C.addressof(hs)
            c.d_glwe_acc, c.d_glwe_bit = ga.data_ptr(), gb.data_ptr()
            out.append((ga, gb))
        _lib.check(self._L.fhe_search_seeded_queries_group_gens_batch(self._grp, arr, len(items),
                                                                      _stream(self.device)))
        return out

    # ------------------------- both-private search for a group (§8.14) --
    def _ggsw_items(self, items):
        """The fhe_group_ggsw array of items (one per engine, None: the tenant
        sits out) whose tuples start (ggsws, base_log, level, docs, B, D); the
        per-tenant Q (0 for None)."""
        if len(items) != len(self.engines):
            raise ValueError(f"{len(items)} items for {len(self.engines)} tenants")
        arr = (_lib.FheGroupGgsw * max(len(items), 1))()
        Qs = []
        for t, (eng, it) in enumerate(zip(self.engines, items)):
            arr[t].struct_size = C.sizeof(_lib.FheGroupGgsw)
            if it is None:
                Qs.append(0)
                continue
            ggsws, base_log, level, docs, B, D = it[:6]
            try:
                Q = eng._ggsws(ggsws, base_log, level)
            except ValueError as e:
                raise ValueError(f"tenant {t}: {e}") from None
            a = arr[t]
            a.D, a.base_log, a.level, a.Q, a.B = int(D), int(base_log), int(level), Q, int(B)
            a.d_ggsw, a.d_docs = ggsws.data_ptr(), docs.data_ptr()
            Qs.append(Q)
        return arr, Qs

    def linear_ggsws(self, items, csts, out: torch.Tensor | None = None) -> torch.Tensor:
        """fhe_linear_ggsws_group_batch. items: one per engine, None (the
        tenant sits this call out) or (ggsws, base_log, level, docs, B, D) as
        Engine.linear_ggsws takes them; csts: per tenant its Q host constants
        (None for a tenant sitting out). Returns the M padded rows of
        rows([Q_t B_t]), kN + 1 words each, the padding rows unwritten
        (`out`: a buffer of at least M rows to write into)."""
        arr, Qs = self._ggsw_items(items)
        if len(csts) != len(items):
            raise ValueError(f"{len(csts)} constant lists for {len(items)} tenants")
        keep, ptrs = [], (C.c_void_p * max(len(items), 1))()
        for t, (Q, cs) in enumerate(zip(Qs, csts)):
            if not Q:
                continue
            k, _ = Engine._i64s(cs)
            if k.size != Q:
                raise ValueError(f"tenant {t}: {k.size} constants for {Q} queries")
            keep.append(k)
            ptrs[t] = k.ctypes.data
        M, _ = group_rows([Q * int(it[4]) if it is not None else 0 for Q, it in zip(Qs, items)])
        if out is not None and out.numel() < M * self.W:
            raise ValueError(f"out holds {out.numel() // self.W} rows, the layout {M}")
        rows = torch.empty((M, self.W), dtype=torch.int64, device=self.device) if out is None else out
        _lib.check(self._L.fhe_linear_ggsws_group_batch(self._grp, arr, len(items), ptrs, _ptr(rows),
                                                        _stream(self.device)))
        return rows

    def search_ggsws(self, items) -> list:
        """fhe_search_ggsws_group_batch. items: one per engine, None (the
        tenant sits this call out) or the arguments of Engine.search_ggsws as
        a tuple (ggsws, base_log, level, docs, B, D, cst, Ts, levels_bit); the
        participating tenants share the gadget level. Returns, per tenant,
        (glwe_acc, glwe_bit) or None."""
        arr, Qs = self._ggsw_items(items)
        keep, out = [], []
        for t, (eng, it, Q) in enumerate(zip(self.engines, items, Qs)):
            if it is None:
                out.append(None)
                continue
            B, cst, Ts, levels_bit = it[4], it[6], it[7], it[8]
            hT, _ = Engine._i64s(Ts)
            if hT.size != Q:
                raise ValueError(f"tenant {t}: {hT.size} thresholds for {Q} queries")
            shape = (eng.glwe_count(Q * int(B)), (eng.params.k + 1) * eng.params.N)
            ga = torch.empty(shape, dtype=torch.int64, device=self.device)
            gb = torch.empty(shape, dtype=torch.int64, device=self.device)
            keep.append(hT)
            a = arr[t]
            a.cst, a.levels_bit, a.h_T = int(cst), int(levels_bit), hT.ctypes.data
            a.d_glwe_acc, a.d_glwe_bit = ga.data_ptr(), gb.data_ptr()
            out.append((ga, gb))
        _lib.check(self._L.fhe_search_ggsws_group_batch(self._grp, arr, len(items), _stream(self.device)))
        return out


def u64(t: torch.Tensor) -> np.ndarray:
    """Device int64 tensor -> host uint64 array (bit pattern)."""
    return t.detach().cpu().numpy().view(np.uint64)
