"""Numpy restatement of the both-private search's seeded payloads (DESIGN.md
§8.15): the mask polynomials of a document GLWE and of a GGSW query from the
ChaCha20 streams of a public mask key, and the expansion of bodies to the full
forms tests/extprod_ref.py works on. The stream is the oracle's block function
(oracle/tfhe_ref.py chacha20_block, pinned to RFC 8439 in
tests/test_oracle_tfhe.py): u64 word w of stream (tag, id) is 32-bit words
2 (w % 8) and 2 (w % 8) + 1 of block w // 8 under nonce (tag, id_lo, id_hi).

  document GLWE g, component i < k:  words [iN, (i+1)N) of (TAG_ENC_MASK, id0 + g)
  GGSW row r = c L + l, component c': words [0, N) of (TAG_GGSW_MASK, id0 + r k + c')
"""
import numpy as np

from oracle import tfhe_ref

from pack_ref import decompose_ks_np

U = np.uint64
M64 = (1 << 64) - 1
TAG_ENC_MASK, TAG_ENC_NOISE, TAG_GGSW_MASK, TAG_GGSW_NOISE = 7, 8, 31, 32


def stream_words(key, tag: int, ident: int, w0: int, n: int) -> np.ndarray:
    """Words [w0, w0 + n) of stream (tag, ident mod 2^64) under the 8-word key; 8 | w0, 8 | n."""
    assert w0 % 8 == 0 and n % 8 == 0
    ident &= M64
    nonce = np.array([tag, ident & 0xFFFFFFFF, ident >> 32], np.uint32)
    out = np.empty(n, U)
    for b in range(n // 8):
        o = tfhe_ref.chacha20_block(key, w0 // 8 + b, nonce).astype(U)
        out[8 * b:8 * b + 8] = o[0::2] | (o[1::2] << U(32))
    return out


def glwe_masks(mask_key, id0: int, G: int, N: int, k: int) -> np.ndarray:
    """[G, k, N]: the masks of document GLWEs id0 .. id0 + G - 1 (modulo 2^64)."""
    return np.stack([stream_words(mask_key, TAG_ENC_MASK, id0 + g, 0, k * N).reshape(k, N) for g in range(G)])


def ggsw_masks(mask_key, id0: int, N: int, k: int, L: int) -> np.ndarray:
    """[(k+1) L, k, N]: the masks of one GGSW's rows."""
    return np.stack([np.stack([stream_words(mask_key, TAG_GGSW_MASK, id0 + r * k + cp, 0, N) for cp in range(k)])
                     for r in range((k + 1) * L)])


def expand_glwe(body, mask_key, id0: int, N: int, k: int) -> np.ndarray:
    """Seeded document bodies [G, N] -> full-form GLWEs [G, k+1, N]."""
    body = np.asarray(body, dtype=U).reshape(-1, N)
    return np.concatenate([glwe_masks(mask_key, id0, len(body), N, k), body[:, None, :]], axis=1)


def expand_ggsw(body, mask_key, id0: int, N: int, k: int, L: int) -> np.ndarray:
    """A seeded query's bodies [(k+1) L, N] -> the full-form GGSW [k+1, L, k+1, N]."""
    body = np.asarray(body, dtype=U).reshape((k + 1) * L, N)
    g = np.concatenate([ggsw_masks(mask_key, id0, N, k, L), body[:, None, :]], axis=1)
    return g.reshape(k + 1, L, k + 1, N)


def digit_signs(words, beta: int, L: int):
    """Per level, whether the balanced digits of `words` take a negative and a positive value."""
    d = decompose_ks_np(np.asarray(words, dtype=U).reshape(1, -1), beta, L)[0]      # [n, L]
    return (d < 0).any(axis=0), (d > 0).any(axis=0)
