"""Numpy restatement of the LWE -> GLWE packing key switch,
shared by tests/test_pack_cpu.py (which pins it against the oracle's
decompose_ks, negacyclic_mul and tuniform) and tests/test_gpu_pack.py (which
compares libfheicp against it word for word). All arithmetic modulo 2^64."""
import numpy as np

U = np.uint64


def decompose_ks_np(x, beta: int, L: int) -> np.ndarray:
    """oracle.tfhe_ref.decompose_ks on an array: int64 digits [..., L], level
    1 first; balanced in [-B/2, B/2], a tie at B/2 decided by input bit
    62 - beta L - (L - l)."""
    x = np.asarray(x, dtype=U)
    prec = L * beta
    v = ((x >> U(63 - prec)) + U(1)) >> U(1)
    B, half = U(1 << beta), U(1 << (beta - 1))
    d = np.zeros(x.shape + (L,), np.int64)
    for l in range(L, 0, -1):
        low = v & (B - U(1))
        v = v >> U(beta)
        coin = (x >> U(62 - prec - (L - l))) & U(1)
        neg = (low > half) | ((low == half) & (coin == U(1)))
        d[..., l - 1] = low.astype(np.int64) - (neg.astype(np.int64) << beta)
        v = v + neg.astype(U)
    return d


def tuniform_np(w, b: int) -> np.ndarray:
    """oracle tuniform on an array of stream words."""
    w = np.asarray(w, dtype=U)
    bits = w & U((2 << (b + 1)) - 1)
    return ((bits >> U(1)) + (bits & U(1))).astype(np.int64) - (1 << b)


def negacyclic_matrix(s, N: int) -> np.ndarray:
    """T with (a * s)[t] = sum_u a[u] T[u, t]: T[u, t] = s[t - u], or
    -s[t - u + N] when t < u."""
    s = np.asarray(s, dtype=U)
    u, t = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    with np.errstate(over="ignore"):
        return np.where(t >= u, s[(t - u) % N], U(0) - s[(t - u) % N])


def glwe_phase(glwe, s_big, N: int, k: int) -> np.ndarray:
    """B - sum_c A_c S_c for GLWEs [G, k+1, N] under S_c[t] = s_big[cN + t]."""
    glwe = np.asarray(glwe, dtype=U).reshape(-1, k + 1, N)
    with np.errstate(over="ignore"):
        ph = glwe[:, k, :].copy()
        for c in range(k):
            ph -= glwe[:, c, :] @ negacyclic_matrix(s_big[c * N:(c + 1) * N], N)
    return ph


def make_pack_key(rng, s_big, N: int, k: int, beta: int, L: int, noise_bits: int) -> np.ndarray:
    """Packing key [kN, L, k+1, N]: row (i, l) a GLWE encryption of the
    constant s_big[i] 2^(64 - beta l), uniform masks, TUniform(noise_bits) noise."""
    big = k * N
    pk = np.zeros((big * L, k + 1, N), U)
    pk[:, :k, :] = rng.integers(0, 2 ** 64, (big * L, k, N), dtype=U)
    e = tuniform_np(rng.integers(0, 2 ** 64, (big * L, N), dtype=U), noise_bits)
    with np.errstate(over="ignore"):
        body = e.astype(U)
        for c in range(k):
            body += pk[:, c, :] @ negacyclic_matrix(s_big[c * N:(c + 1) * N], N)
        msg = np.array([[(int(s_big[i]) << (64 - beta * (l + 1))) % 2 ** 64 for l in range(L)] for i in range(big)], U)
        body[:, 0] += msg.reshape(-1)
    pk[:, k, :] = body
    return pk.reshape(big, L, k + 1, N)


def gemm_rows(ct, pk, beta: int, levels: int) -> np.ndarray:
    """M[j] = -sum_i sum_{l <= levels} d_{j,i,l} PK[i][l] as [count, k+1, N]."""
    ct = np.asarray(ct, dtype=U)
    big, _, k1, N = pk.shape
    d = decompose_ks_np(ct[:, :big], beta, levels)                  # [count, big, levels]
    with np.errstate(over="ignore"):
        m = d.reshape(len(ct), big * levels).astype(U) @ pk[:, :levels].reshape(big * levels, k1 * N)
        return (U(0) - m).reshape(len(ct), k1, N)


def rotate_sum(M, bodies, N: int) -> np.ndarray:
    """sum_j X^j [(0, .., 0, b_j) + M[j]] for j < len(M) <= N, negacyclic: [k+1, N]."""
    out = np.zeros(M.shape[1:], U)
    with np.errstate(over="ignore"):
        for j in range(len(M)):
            r = np.roll(M[j], j, axis=-1)
            r[:, :j] = U(0) - r[:, :j]
            out += r
            out[-1, j] += bodies[j]
    return out


def pack_from_rows(M, ct, count: int, N: int) -> np.ndarray:
    """The packed GLWEs [ceil(count / N), k+1, N] of the first `count` inputs."""
    ct = np.asarray(ct, dtype=U)
    return np.stack([rotate_sum(M[g:min(g + N, count)], ct[g:min(g + N, count), -1], N)
                     for g in range(0, count, N)])


def pack_ref(ct, pk, beta: int, levels: int) -> np.ndarray:
    N = pk.shape[3]
    return pack_from_rows(gemm_rows(ct, pk, beta, levels), ct, len(ct), N)


def pack_var(p, count: int, beta: int, L: int) -> float:
    """The issue's model, recomputed here (integer-word units)."""
    B = 2.0 ** beta
    kN = p.k * p.N
    tv = (2.0 ** (2 * p.glwe_noise_bits + 1) + 1.0) / 6.0
    return min(count, p.N) * kN * L * ((B * B + 2) / 12.0) * tv + (1 + kN / 2) * 2.0 ** (2 * (64 - beta * L)) / 12.0
