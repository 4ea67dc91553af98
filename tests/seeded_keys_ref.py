"""Numpy restatement of the seeded evaluation keys: a key as
the body of every row and the public mask key, and the two expansions back to
the standard form. The stream is the oracle's block function
(oracle/tfhe_ref.py chacha20_block, pinned to RFC 8439 in
tests/test_oracle_tfhe.py): u64 word w of stream (tag, id) is 32-bit words
2 (w % 8) and 2 (w % 8) + 1 of block w // 8 under nonce (tag, id_lo, id_hi).

  GLWE rows (bsk, a gadget's key, the packing key): row r of (k+1) N words is,
    for c < k, words [0, N) of (tag, r k + c), then the N body words of row r;
  LWE rows (ksk, the bridge key): row r of n1 words is words [0, n1 - 1) of
    (tag, r), then body word r.

The one-key keygen's bootstrapping keys are not of that form: a GGSW row with
c < k carries its message on a mask word. messages_to_body restates the move
the seeded keygen makes instead (same streams, same noise, same phase).
"""
import numpy as np

from oracle import tfhe_ref

U = np.uint64
TAG_BSK_MASK, TAG_KSK_MASK, TAG_PACK_MASK, TAG_BRIDGE_MASK = 3, 5, 29, 33
#: gadget g = 1..5 (fast, fast2, mid, mid2, mid0): the mask tag of its classic and of its multi-bit key
TAG_GADGET_MASK = {1: 9, 2: 11, 3: 17, 4: 19, 5: 25}
TAG_MB_MASK = {1: 13, 2: 15, 3: 21, 4: 23, 5: 27}


def stream_head(key, tag: int, ident: int, n: int) -> np.ndarray:
    """Words [0, n) of stream (tag, ident) under the 8-word key; the last block may be partly used."""
    nonce = np.array([tag, ident & 0xFFFFFFFF, ident >> 32], np.uint32)
    out = np.empty(8 * (-(-n // 8)), U)
    for b in range(out.size // 8):
        o = tfhe_ref.chacha20_block(key, b, nonce).astype(U)
        out[8 * b:8 * b + 8] = o[0::2] | (o[1::2] << U(32))
    return out[:n]


def glwe_row_bodies(key, N: int, k: int) -> np.ndarray:
    """A GLWE-row key in standard form -> its bodies [rows, N]."""
    return np.asarray(key, dtype=U).reshape(-1, (k + 1) * N)[:, k * N:].copy()


def lwe_row_bodies(key, n1: int) -> np.ndarray:
    """An LWE-row key in standard form -> its bodies [rows]."""
    return np.asarray(key, dtype=U).reshape(-1, n1)[:, n1 - 1].copy()


def glwe_row(body_row, mask_key, tag: int, r: int, N: int, k: int) -> np.ndarray:
    """Row r of a GLWE-row key, (k+1) N words, from its N body words."""
    return np.concatenate([stream_head(mask_key, tag, r * k + c, N) for c in range(k)] +
                          [np.asarray(body_row, dtype=U).reshape(N)])


def lwe_row(body_word, mask_key, tag: int, r: int, n1: int) -> np.ndarray:
    """Row r of an LWE-row key, n1 words, from its body word."""
    return np.concatenate([stream_head(mask_key, tag, r, n1 - 1), np.array([body_word], U)])


def expand_glwe_rows(body, mask_key, tag: int, N: int, k: int) -> np.ndarray:
    """Bodies [rows, N] -> the key in standard form, flat."""
    body = np.asarray(body, dtype=U).reshape(-1, N)
    return np.concatenate([glwe_row(body[r], mask_key, tag, r, N, k) for r in range(len(body))])


def expand_lwe_rows(body, mask_key, tag: int, n1: int) -> np.ndarray:
    """Bodies [rows] -> the key in standard form, flat."""
    body = np.asarray(body, dtype=U).reshape(-1)
    return np.concatenate([lwe_row(body[r], mask_key, tag, r, n1) for r in range(body.size)])


def gadget_tag(params, g: int) -> int:
    """The mask tag of gadget g's key under these parameters (multi-bit when its group is 2)."""
    grp = {1: params.pbs_fast_group, 2: params.pbs_fast2_group, 3: params.pbs_mid_group, 4: params.pbs_mid2_group,
           5: params.pbs_mid0_group}[g]
    return TAG_MB_MASK[g] if grp == 2 else TAG_GADGET_MASK[g]


def expand_eval_keys(d: dict, params) -> dict:
    """A seeded evaluation-key dict -> the full-form arrays it stands for
    (bsk, ksk, gadget_bsk{g}, pack_key, bridge_key where present)."""
    N, k, n = params.N, params.k, params.n
    mk = np.asarray(d["eval_mask_key"], np.uint32)
    out = {"bsk": expand_glwe_rows(d["bsk_body"], mk, TAG_BSK_MASK, N, k),
           "ksk": expand_lwe_rows(d["ksk_body"], mk, TAG_KSK_MASK, n + 1)}
    for g in (1, 2, 3, 4, 5):
        if f"gadget_bsk{g}_body" in d:
            out[f"gadget_bsk{g}"] = expand_glwe_rows(d[f"gadget_bsk{g}_body"], mk, gadget_tag(params, g), N, k)
    if "pack_key_body" in d:
        out["pack_key"] = expand_glwe_rows(d["pack_key_body"], np.asarray(d["pack_mask_key"], np.uint32),
                                           TAG_PACK_MASK, N, k)
    if "bridge_key_body" in d:
        out["bridge_key"] = expand_lwe_rows(d["bridge_key_body"], np.asarray(d["bridge_mask_key"], np.uint32),
                                            TAG_BRIDGE_MASK, k * N + 1)
    return out


def mb_messages(s_small) -> np.ndarray:
    """The GGSW messages of a multi-bit key: per pair (s1, s2)
    of the small secret (s2 = 0 past n) the indicators s1 (1 - s2), (1 - s1) s2, s1 s2."""
    s = np.asarray(s_small, dtype=np.int64).reshape(-1)
    s = np.concatenate([s, np.zeros(s.size % 2, np.int64)]).reshape(-1, 2)
    return np.stack([s[:, 0] * (1 - s[:, 1]), (1 - s[:, 0]) * s[:, 1], s[:, 0] * s[:, 1]], axis=1).reshape(-1)


def messages_to_body(key, msgs, s_big, N: int, k: int, L: int, beta: int) -> np.ndarray:
    """A bootstrapping key as the one-key keygen writes it -> as the seeded
    keygen writes it under the same streams. GGSW i, row r = c L + (l - 1),
    g = 2^(64 - l beta): for c < k and msgs[i] = 1 the one-key form has g on
    word cN of the mask; the seeded form keeps the mask a pure stream word and
    has -g S_c on the body (phase e - g S_c in both). Rows c = k are the same."""
    key = np.asarray(key, dtype=U).reshape(len(msgs), k + 1, L, k + 1, N).copy()
    S = np.asarray(s_big, dtype=U).reshape(k, N)
    with np.errstate(over="ignore"):
        for i in np.flatnonzero(np.asarray(msgs)):
            for c in range(k):
                for l in range(1, L + 1):
                    g = U(1) << U(64 - l * beta)
                    key[i, c, l - 1, c, 0] -= g
                    key[i, c, l - 1, k] -= g * S[c]
    return key.reshape(-1)


def lwe_row_phases(key, n1: int, secret) -> np.ndarray:
    """b - <a, s> mod 2^64 of every row of an LWE-row key (secret: n1 - 1 words of 0/1)."""
    rows = np.asarray(key, dtype=U).reshape(-1, n1)
    s = np.asarray(secret, dtype=U).reshape(-1)
    with np.errstate(over="ignore"):
        return rows[:, n1 - 1] - (rows[:, :n1 - 1] * s[None, :]).sum(axis=1, dtype=U)
