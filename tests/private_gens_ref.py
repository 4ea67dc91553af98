"""Numpy restatement of the both-private search over several key generations
(DESIGN.md §8.19): per generation tests/extprod_ref.py's leveled step on that
generation's documents and GGSWs, the rows laid out query-major over all
generations, then tests/bridge_ref.py's bridge on every old generation's rows
with that generation's key. Shared by tests/test_private_gens_cpu.py and
tests/test_gpu_private_gens.py, which compares libfheicp against it word for
word. All arithmetic modulo 2^64."""
import numpy as np

import bridge_ref as BR
import extprod_ref as X
from pack_ref import negacyclic_matrix, tuniform_np

U = np.uint64


def offsets(Bs) -> list:
    """off_g = sum_{h<g} B_h."""
    return [int(sum(Bs[:g])) for g in range(len(Bs))]


def gen_rows(Qn: int, Bs, g: int) -> np.ndarray:
    """Rows {q B + off_g + b} of generation g in (q, b) order: the compact
    order of that generation's own Q x B_g result."""
    B, off = int(sum(Bs)), offsets(Bs)[g]
    return np.array([q * B + off + b for q in range(Qn) for b in range(Bs[g])], dtype=np.int64)


def scatter_gens(per_gen, Qn: int, Bs, width: int) -> np.ndarray:
    """per_gen[g]: generation g's compact [Q B_g, width] rows (None where
    B_g = 0) -> the call's [Q B, width] matrix."""
    out = np.zeros((Qn * int(sum(Bs)), width), U)
    for g, rows in enumerate(per_gen):
        if Bs[g]:
            out[gen_rows(Qn, Bs, g)] = np.asarray(rows, dtype=U).reshape(Qn * Bs[g], width)
    return out


def linear_gens_ref(glwes, ggsws, Bs, beta: int, D: int, csts, msg_bits: int) -> np.ndarray:
    """glwes[g] [G_g, k+1, N], ggsws[g] [Q, k+1, L, k+1, N]: row q B + off_g + b
    is linear_ggsw_ref of generation g's document b under generation g's
    query q with csts[q] on the body."""
    Qn = len(csts)
    per = []
    for g, Bg in enumerate(Bs):
        if not Bg:
            per.append(None)
            continue
        per.append(np.concatenate([X.linear_ggsw_ref(glwes[g], ggsws[g][q], beta, Bg, D, int(csts[q]), msg_bits)
                                   for q in range(Qn)]))
    width = next(p.shape[1] for p in per if p is not None)
    return scatter_gens(per, Qn, Bs, width)


def bridge_gens_ref(rows, Qn: int, Bs, keys, beta: int, levels: int) -> np.ndarray:
    """bridge_ref on the rows of every generation g with keys[g] not None;
    the other rows (the current generation's) unchanged."""
    out = np.array(rows, dtype=U, copy=True)
    for g, bk in enumerate(keys):
        if bk is not None and Bs[g]:
            idx = gen_rows(Qn, Bs, g)
            out[idx] = BR.bridge_ref(out[idx], bk, beta, levels)
    return out


def encrypt_docs_glwe(rng, dq, s_big, N: int, k: int, P: int, noise_bits: int) -> np.ndarray:
    """Quantized documents [B, D] -> GLWEs [G, k+1, N] under s_big, S = N // D
    documents per GLWE, feature j of document i at coefficient i D + j,
    Delta = 2^(64 - P), uniform masks, TUniform(noise_bits) noise."""
    rows = X.pack_docs_rows(dq, N)
    G = len(rows)
    s_big = np.asarray(s_big, dtype=U)
    glwe = np.zeros((G, k + 1, N), U)
    glwe[:, :k] = rng.integers(0, 2 ** 64, (G, k, N), dtype=U)
    with np.errstate(over="ignore"):
        body = tuniform_np(rng.integers(0, 2 ** 64, (G, N), dtype=U), noise_bits).astype(U)
        for c in range(k):
            body += glwe[:, c] @ negacyclic_matrix(s_big[c * N:(c + 1) * N], N)
        body[:, :rows.shape[1]] += rows.astype(U) << U(64 - P)
    glwe[:, k] = body
    return glwe


def encrypt_ggsw(rng, W, s_big, N: int, k: int, beta: int, L: int, noise_bits: int) -> np.ndarray:
    rows = (k + 1) * L
    return X.make_ggsw(rng.integers(0, 2 ** 64, (rows, k, N), dtype=U), rng.integers(0, 2 ** 64, (rows, N), dtype=U),
                       W, s_big, N, k, beta, L, noise_bits)
