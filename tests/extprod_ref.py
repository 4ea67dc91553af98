"""Numpy restatement of the both-private search's leveled step (DESIGN.md
§8.7): GGSW rows of the sparse query polynomial, the exact external product
with a document GLWE and the slot extraction. Built on tests/pack_ref.py's
decompose_ks_np / negacyclic_matrix (pinned to the oracle there and in
tests/test_extprod_cpu.py); tests/test_gpu_extprod.py compares libfheicp
against it word for word. All arithmetic modulo 2^64."""
import numpy as np

from pack_ref import decompose_ks_np, negacyclic_matrix, tuniform_np

U = np.uint64


def query_poly(W, N: int) -> np.ndarray:
    """Q = sum_j W_j X^-j = W_0 - sum_{j >= 1} W_j X^(N - j) as N words."""
    W = np.asarray(W, dtype=np.int64)
    q = np.zeros(N, U)
    with np.errstate(over="ignore"):
        q[0] = W[0].astype(U)
        for j in range(1, len(W)):
            q[N - j] = U(0) - W[j].astype(U)
    return q


def ggsw_messages(W, s_big, N: int, k: int, beta: int, L: int) -> np.ndarray:
    """[k+1, L, N]: Q 2^(64 - beta l) for c = k, -S_c Q 2^(64 - beta l) for c < k."""
    q = query_poly(W, N)
    s_big = np.asarray(s_big, dtype=U)
    out = np.zeros((k + 1, L, N), U)
    with np.errstate(over="ignore"):
        for c in range(k + 1):
            m = q if c == k else U(0) - s_big[c * N:(c + 1) * N] @ negacyclic_matrix(q, N)
            for l in range(L):
                out[c, l] = m << U(64 - beta * (l + 1))
    return out


def make_ggsw(masks, noise_words, W, s_big, N: int, k: int, beta: int, L: int, noise_bits: int) -> np.ndarray:
    """GGSW [k+1, L, k+1, N] from given masks [(k+1) L, k, N] and noise stream
    words [(k+1) L, N]: body = sum_c A_c S_c + TUniform(noise) + message."""
    s_big = np.asarray(s_big, dtype=U)
    rows = (k + 1) * L
    g = np.zeros((rows, k + 1, N), U)
    g[:, :k] = np.asarray(masks, dtype=U).reshape(rows, k, N)
    with np.errstate(over="ignore"):
        body = tuniform_np(np.asarray(noise_words, dtype=U).reshape(rows, N), noise_bits).astype(U)
        for c in range(k):
            body += g[:, c] @ negacyclic_matrix(s_big[c * N:(c + 1) * N], N)
        body += ggsw_messages(W, s_big, N, k, beta, L).reshape(rows, N)
    g[:, k] = body
    return g.reshape(k + 1, L, k + 1, N)


def toeplitz(ggsw) -> np.ndarray:
    """The GEMM's right operand [(k+1) N L, (k+1) N], K level-major:
    T[l (k+1)N + cN + u][c' N + t] = +-Row(c, l)[c'][(t - u) mod N], minus when t < u."""
    k1, L, _, N = ggsw.shape
    T = np.zeros((L, k1, N, k1, N), U)
    for c in range(k1):
        for l in range(L):
            for cp in range(k1):
                T[l, c, :, cp, :] = negacyclic_matrix(ggsw[c, l, cp], N)
    return T.reshape(L * k1 * N, k1 * N)


def external_product(glwe, ggsw, beta: int) -> np.ndarray:
    """out_g = sum_c sum_l d_{g,c,l}(X) Row(c, l) for GLWEs [G, k+1, N]: [G, k+1, N]."""
    k1, L, _, N = ggsw.shape
    glwe = np.asarray(glwe, dtype=U).reshape(-1, k1 * N)
    d = decompose_ks_np(glwe, beta, L)                                  # [G, (k+1)N, L]
    dl = np.moveaxis(d, 2, 1).reshape(len(glwe), L * k1 * N)            # level-major
    with np.errstate(over="ignore"):
        return (dl.astype(U) @ toeplitz(ggsw)).reshape(len(glwe), k1, N)


def extract_slots(out, B: int, D: int, cst_scaled: int) -> np.ndarray:
    """Sample extraction of coefficient (b % S) D of GLWE b // S, S = N // D,
    with cst_scaled on the body: big LWEs [B, kN + 1]."""
    G, k1, N = out.shape
    k, S = k1 - 1, N // D
    lwe = np.zeros((B, k * N + 1), U)
    with np.errstate(over="ignore"):
        for b in range(B):
            g, p = divmod(b, S)
            p *= D
            for c in range(k):
                a = out[g, c]
                lwe[b, c * N:c * N + p + 1] = a[p::-1]                  # u <= p: A_c[p - u]
                lwe[b, c * N + p + 1:(c + 1) * N] = U(0) - a[:p:-1]     # u > p: -A_c[p - u + N]
            lwe[b, k * N] = out[g, k, p] + U(cst_scaled % 2 ** 64)
    return lwe


def linear_ggsw_ref(glwe, ggsw, beta: int, B: int, D: int, cst: int, msg_bits: int) -> np.ndarray:
    return extract_slots(external_product(glwe, ggsw, beta), B, D, (cst << (64 - msg_bits)) % 2 ** 64)


def lwe_phase(lwe, s_big) -> np.ndarray:
    lwe = np.asarray(lwe, dtype=U)
    with np.errstate(over="ignore"):
        return lwe[:, -1] - lwe[:, :-1] @ np.asarray(s_big, dtype=U)


def pack_docs_rows(dq, N: int) -> np.ndarray:
    """Quantized documents [B, D] -> rows of S D values, [G, S D] (zero padded)."""
    dq = np.asarray(dq, dtype=np.int64)
    B, D = dq.shape
    S = N // D
    G = -(-B // S)
    rows = np.zeros((G * S, D), np.int64)
    rows[:B] = dq
    return rows.reshape(G, S * D)


def extprod_var(p, w2: float, beta: int, L: int) -> float:
    """The issue's model, recomputed here (integer-word units)."""
    B = 2.0 ** beta
    tv = (2.0 ** (2 * p.glwe_noise_bits + 1) + 1.0) / 6.0
    return (w2 * tv + (p.k + 1) * L * p.N * ((B * B + 2) / 12.0) * tv
            + w2 * (1 + p.k * p.N / 2) * 2.0 ** (2 * (64 - beta * L)) / 12.0)
