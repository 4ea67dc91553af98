"""Numpy restatement of the LWE -> LWE bridge key switch of a key rotation
(DESIGN.md §8.12), built on tests/pack_ref.py's decompose_ks_np and
tuniform_np (which tests/test_pack_cpu.py pins to the oracle). Shared by
tests/test_bridge_cpu.py and tests/test_gpu_bridge.py, which compares
libfheicp against it word for word. All arithmetic modulo 2^64."""
import numpy as np

from pack_ref import decompose_ks_np, tuniform_np

U = np.uint64


def make_bridge_key(rng, s_old, s_new, beta: int, L: int, noise_bits: int) -> np.ndarray:
    """Bridge key [kN, L, kN+1]: row (i, l) an LWE under s_new of the constant
    s_old[i] 2^(64 - beta l), uniform masks, TUniform(noise_bits) noise."""
    s_old, s_new = np.asarray(s_old, dtype=U), np.asarray(s_new, dtype=U)
    big = s_old.size
    bk = np.zeros((big * L, big + 1), U)
    bk[:, :big] = rng.integers(0, 2 ** 64, (big * L, big), dtype=U)
    e = tuniform_np(rng.integers(0, 2 ** 64, big * L, dtype=U), noise_bits)
    msg = np.array([[(int(s_old[i]) << (64 - beta * (l + 1))) % 2 ** 64 for l in range(L)] for i in range(big)], U)
    with np.errstate(over="ignore"):
        bk[:, big] = bk[:, :big] @ s_new + e.astype(U) + msg.reshape(-1)
    return bk.reshape(big, L, big + 1)


def bridge_ref(ct, bk, beta: int, levels: int, cols=None) -> np.ndarray:
    """out = (0, .., 0, b) - sum_i sum_l d_{i,l} BK[i][l] for each row of ct
    [count, kN+1]; bk [kN, levels, kN+1]. cols: only these output columns
    (the body column is kN)."""
    ct = np.asarray(ct, dtype=U)
    big = bk.shape[0]
    d = decompose_ks_np(ct[:, :big], beta, levels)                      # [count, big, levels]
    key = bk.reshape(big * levels, big + 1)
    idx = np.arange(big + 1) if cols is None else np.asarray(cols)
    with np.errstate(over="ignore"):
        out = U(0) - d.reshape(len(ct), big * levels).astype(U) @ key[:, idx]
        out[:, idx == big] += ct[:, big:big + 1]
    return out


def lwe_phase(ct, s) -> np.ndarray:
    """b - a . s for rows of ct [count, n+1]."""
    ct, s = np.asarray(ct, dtype=U), np.asarray(s, dtype=U)
    with np.errstate(over="ignore"):
        return ct[:, -1] - ct[:, :-1] @ s


def bridge_phase_ref(ct, bk, s_new, beta: int, levels: int) -> np.ndarray:
    """lwe_phase(bridge_ref(ct), s_new) without forming the mask columns:
    b - sum d_{i,l} phase(BK[i][l])."""
    ct = np.asarray(ct, dtype=U)
    big = bk.shape[0]
    d = decompose_ks_np(ct[:, :big], beta, levels)
    kp = lwe_phase(bk.reshape(big * levels, big + 1), s_new)
    with np.errstate(over="ignore"):
        return ct[:, big] - d.reshape(len(ct), big * levels).astype(U) @ kp


def encrypt_lwe(rng, msgs, s, P: int, noise_bits: int) -> np.ndarray:
    """Big LWEs [count, n+1] of signed P-bit messages under s (Delta = 2^(64 - P))."""
    s = np.asarray(s, dtype=U)
    m = np.asarray(msgs, dtype=np.int64)
    ct = np.zeros((m.size, s.size + 1), U)
    ct[:, :-1] = rng.integers(0, 2 ** 64, (m.size, s.size), dtype=U)
    e = tuniform_np(rng.integers(0, 2 ** 64, m.size, dtype=U), noise_bits)
    with np.errstate(over="ignore"):
        ct[:, -1] = ct[:, :-1] @ s + e.astype(U) + (m.astype(U) << U(64 - P))
    return ct


def decode(phase, P: int) -> np.ndarray:
    q = ((np.asarray(phase, dtype=U) >> U(63 - P)) + U(1)) >> U(1)
    q = (q & U((1 << P) - 1)).astype(np.int64)
    return np.where(q >= 1 << (P - 1), q - (1 << P), q)


def bridge_var(p, beta: int, L: int) -> float:
    """The issue's model, recomputed here (integer-word units): pack_var at count 1."""
    B = 2.0 ** beta
    kN = p.k * p.N
    tv = (2.0 ** (2 * p.glwe_noise_bits + 1) + 1.0) / 6.0
    return kN * L * ((B * B + 2) / 12.0) * tv + (1 + kN / 2) * 2.0 ** (2 * (64 - beta * L)) / 12.0
