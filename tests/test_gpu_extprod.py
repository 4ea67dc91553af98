"""GPU: the both-private search through libfheicp.

The GGSW encryption of the query polynomial, the leveled step (document
digits, Toeplitz byte planes, the i8 MFMA GEMM, slot extraction) word for word
against the numpy restatement (tests/extprod_ref.py), the decrypted results
against the clear sums, the single-party compare and the evaluation-only
search against the private-query path and the oracle's restatement
(quant_ref.corpus_*), and the extracted-phase noise at the real parameters
against the model."""
import math

import numpy as np
import pytest
import torch

import extprod_ref as X
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine, u64
from fheicp.params import TOY, extprod_plan, extprod_var, params_for_bits

pytestmark = pytest.mark.gpu

U = np.uint64
GADGETS = [(4, 3), (7, 7)]
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0, 1 << 63)
W16 = np.array([3, -2, 0, 7, -128 * 31, 0, 1, -1, 5, 0, -9, 127 * 31, 2, -4, 0, 6], np.int64)


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(eng.device)


@pytest.fixture(scope="module")
def toy(need_gpu):
    eng = Engine(TOY, 0)
    eng.keygen(99)
    return eng, eng.export_keys()["s_big"].astype(U)


@pytest.mark.parametrize("gadget", GADGETS)
@pytest.mark.parametrize("D", [1, 5, 16, 256])
def test_ggsw_rows_decrypt_to_their_messages(toy, gadget, D):
    """(a) every GPU-made row's raw phase is its message within TUniform's range."""
    eng, s_big = toy
    p = eng.params
    beta, L = gadget
    rng = np.random.default_rng(D)
    W = rng.integers(-2 ** 12, 2 ** 12, D)
    W[0] = -W[0] - 1
    if D > 2:
        W[1], W[D - 1] = 0, -5
    g = eng.encrypt_ggsw(W, beta, L, 1234 + D, id0=7)
    rows = (p.k + 1) * L
    assert g.numel() == eng.ggsw_words(beta, L) == rows * (p.k + 1) * p.N
    ph = u64(eng.decrypt_packed(g, rows * p.N, 2)).reshape(rows, p.N)
    msg = X.ggsw_messages(W, s_big, p.N, p.k, beta, L).reshape(rows, p.N)
    with np.errstate(over="ignore"):
        err = (ph - msg).view(np.int64)
    assert np.abs(err).max() <= 1 << p.glwe_noise_bits
    assert err.std() > 2.0 ** (p.glwe_noise_bits - 2)             # and it is noise, not zeros
    # masks and noise come from the stream id: another id0, other rows
    g2 = eng.encrypt_ggsw(W, beta, L, 1234 + D, id0=8)
    assert not np.array_equal(u64(g2)[0, 0], u64(g)[0, 0])


@pytest.fixture(scope="module")
def exact_ref(toy):
    """Per gadget: a GPU-made GGSW of W16 (negative and zero weights) with edge
    words planted, 17 document GLWEs of arbitrary words, and the restatement's
    external product of all 17, computed once."""
    eng, _ = toy
    p = eng.params
    out = {}
    for beta, L in GADGETS:
        rng = np.random.default_rng(100 * beta + L)
        ggsw = u64(eng.encrypt_ggsw(W16, beta, L, 77, id0=3)).reshape(p.k + 1, L, p.k + 1, p.N).copy()
        for i, w in enumerate(EDGE_WORDS):
            ggsw[i % (p.k + 1), i % L, (i + 1) % (p.k + 1), 3 * i:3 * i + 2] = U(w)
        glwe = rng.integers(0, 2 ** 64, (17, p.k + 1, p.N), dtype=U)
        for i, w in enumerate(EDGE_WORDS):
            glwe[i % 17, i % (p.k + 1), 5 * i:5 * i + 3] = U(w)
        # ties at B/2 on every level, both coins
        prec = beta * L
        ties = [((1 << (beta - 1)) << (64 - beta * l)) | (c << (62 - prec - (L - l))) for l in range(1, L + 1)
                for c in (0, 1)]
        glwe[16, p.k, :len(ties)] = np.array(ties, U)
        out[(beta, L)] = (ggsw, glwe, X.external_product(glwe, ggsw, beta))
    return out


@pytest.mark.parametrize("gadget", GADGETS)
@pytest.mark.parametrize("kind", ["partial", "two", "g17"])
@pytest.mark.parametrize("D", [1, 5, 16, 256])
def test_linear_ggsw_bit_exact(toy, exact_ref, gadget, kind, D):
    """(b) fhe_linear_ggsw_batch equals the restatement word for word."""
    eng, _ = toy
    p = eng.params
    beta, L = gadget
    ggsw, glwe, prod = exact_ref[gadget]
    S = p.N // D
    G = {"partial": 1, "two": 2, "g17": 17}[kind]                  # 17: past one 16-row tile
    B = G * S if S == 1 else (G - 1) * S + max(1, S // 3)           # the last GLWE partly filled
    assert eng.doc_glwes(B, D) == G
    docs8 = eng.pack_docs_glwe(dev_u64(eng, glwe[:G]), B, D, beta, L)
    assert docs8.numel() == -(-G // 16) * 16 * (p.k + 1) * p.N * L
    cst = -37
    got = u64(eng.linear_ggsw(dev_u64(eng, ggsw), beta, L, docs8, B, D, cst))
    want = X.extract_slots(prod[:G], B, D, (cst << (64 - p.msg_bits)) % 2 ** 64)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("D", [1, 5, 16, 256])
def test_linear_ggsw_decrypts_to_clear_sum(toy, D):
    """(c) encrypted documents, an encrypted query: the accumulators decrypt to
    sum_j W_j dq[b, j] + cst (|value| <= 256 * 2 * 4 + 17 < 2^13; the planned
    gadget keeps 2^49 at 9.2 sigma)."""
    eng, _ = toy
    P = 14
    eng.set_msg_bits(P)
    try:
        p = eng.params
        rng = np.random.default_rng(40 + D)
        S = p.N // D
        B = 2 * S + max(1, S // 2) if S > 1 else 3
        dq = rng.integers(-4, 4, (B, D))
        W = rng.integers(-2, 3, D)
        W[0] = -2
        if D > 2:
            W[D // 2] = 0
        cst = -17
        beta, L = extprod_plan(p, float(np.sum(W * W)))
        glwe = eng.encrypt_docs_glwe(dq, 9, id0=100)
        assert glwe.shape == (eng.doc_glwes(B, D), (p.k + 1) * p.N)
        # the packed documents decrypt to themselves, zeros elsewhere
        vals = eng.decrypt_packed(glwe, glwe.shape[0] * p.N, 0).cpu().numpy().reshape(-1, p.N)
        np.testing.assert_array_equal(vals[:, :S * D].reshape(-1, D)[:B], dq)
        assert not vals[:, S * D:].any() and not vals[:, :S * D].reshape(-1, D)[B:].any()
        docs8 = eng.pack_docs_glwe(glwe, B, D, beta, L)
        ggsw = eng.encrypt_ggsw(W, beta, L, 10, id0=5)
        out = eng.linear_ggsw(ggsw, beta, L, docs8, B, D, cst)
        np.testing.assert_array_equal(eng.decrypt(out).cpu().numpy(), dq @ W + cst)
    finally:
        eng.set_msg_bits(TOY.msg_bits)


@pytest.fixture(scope="module")
def private16(need_gpu):
    """The 16-dim, n_bits 6 model of tests/test_gpu_query.py, both modes on it."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.private import PrivateClient
    from fheicp.query import EncryptedQuerySearch
    Xt, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(Xt, y, 6)
    oq = Q.fit_quantized_linear(Xt, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client = PrivateClient(c, count=64, pack_seed=4, enc_seed=12)
    return c, EncryptedQuerySearch(c), client, oq, {}


def test_compare_ggsw_matches_query_path(private16):
    """(d) fhe_compare_ggsw_batch returns the (acc, below) of
    fhe_compare_query_batch and of quant_ref.corpus_*: same model, B = 64,
    a threshold with documents on both sides."""
    c, qs, client, oq, memo = private16
    eng = c.engine
    q, docs = Q.make_corpus(16, 64, seed=21)
    s_e = c.cq.s_e
    ref_acc = Q.corpus_accumulate(oq, s_e, 6, q, docs)
    scores = np.float64(Q.corpus_out_scale(oq, s_e)) * ref_acc.astype(np.float64)
    block = client.encrypt_docs(docs)
    np.testing.assert_array_equal(client.decrypt_docs(block), Q.corpus_quant(s_e, 6, docs))
    payload = client.encrypt_query(q)
    from fheicp.private import unpack_doc_block, unpack_ggsw_query
    bl, pl = unpack_doc_block(block), unpack_ggsw_query(payload)
    assert (pl["base_log"], pl["level"]) == client.gadget == extprod_plan(c.scheme.with_msg_bits(c.P0),
                                                                          _worst(c.cq))
    docs8 = eng.pack_docs_glwe(eng.to_dev(bl["glwe"]), 64, 16, *client.gadget)
    ggsw = eng.to_dev(pl["ggsw"])
    for t in (0.5, float(np.median(scores))):
        _, cst, T = qs.plan(t)
        eng.set_msg_bits(c.P0)
        acc, below = eng.compare_ggsw(ggsw, *client.gadget, docs8, 64, 16, cst, T)
        acc_q, below_q = qs.compare(qs.encrypt_query(q), qs.pack_docs(docs), 64, t)
        np.testing.assert_array_equal(acc.cpu().numpy(), ref_acc)
        np.testing.assert_array_equal(acc.cpu().numpy(), acc_q.cpu().numpy())
        want = (scores < t).astype(np.int64)
        np.testing.assert_array_equal(below.cpu().numpy(), want)
        np.testing.assert_array_equal(below.cpu().numpy(), below_q.cpu().numpy())
    assert 0.25 <= want.mean() <= 0.75
    memo.update(block=block, payload=payload, acc=ref_acc, below=want, t=t)


def _worst(cq):
    from fheicp.private import worst_norm2
    return worst_norm2(cq)


def test_search_ggsw_on_evaluation_only_context(private16):
    """(e) a server with evaluation keys only: the reply decrypts to (d)'s
    values; encrypting there is FHE_E_STATE."""
    from fheicp.private import PrivateServer
    c, qs, client, oq, memo = private16
    if not memo:
        test_compare_ggsw_matches_query_path(private16)
    server = PrivateServer(client.eval_keys(), c.cq, c.P0, device=0, scheme=c.scheme)
    assert (server.base_log, server.level) == client.gadget
    docs8, B = server.pack_docs(memo["block"])
    assert B == 64
    reply = server.search(memo["payload"], docs8, B, memo["t"])
    n1 = (c.scheme.k + 1) * c.scheme.N
    assert reply.size == 4 + 2 * n1
    acc, below = client.decrypt_reply(reply)
    np.testing.assert_array_equal(acc.cpu().numpy(), memo["acc"])
    np.testing.assert_array_equal(below.cpu().numpy(), memo["below"])
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        server.engine.encrypt_ggsw(np.arange(16), *client.gadget, 1)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        server.engine.compare_ggsw(server.engine.to_dev(np.zeros(8, np.int64)), *client.gadget, docs8, B, 16, 0, 0)
    server.engine.close()


def test_extracted_phase_noise_at_real_parameters(private16):
    """P = 16, D = 16, 4096 documents (64 GLWEs), the weights of the 16-dim
    model and the query of (d): the extracted phases' RMS error against the
    model (fhe_extprod_plan's variance at this ||W||^2), as
    tests/test_gpu_noise.py does. Measured on one MI355X: sigma 2^41.94, model
    2^42.43, ratio 0.716 (these weights sum to about 0, where the rounding
    errors' correlation under a binary key predicts sqrt(1/2))."""
    c, _, _, _, _ = private16
    q, _ = Q.make_corpus(16, 64, seed=21)
    W = c.cq.weights(c.cq.quant(q))
    prm = params_for_bits(16)
    eng = Engine(prm, 0)
    eng.keygen(6200)
    w2 = float(np.sum(W.astype(np.float64) ** 2))
    beta, L = extprod_plan(prm, w2)
    rng = np.random.default_rng(16)
    B, D = 4096, 16
    dq = rng.integers(c.cq.qmin, c.cq.qmax + 1, (B, D))
    glwe = eng.encrypt_docs_glwe(dq, 31, id0=0)
    assert glwe.shape[0] == 64
    docs8 = eng.pack_docs_glwe(glwe, B, D, beta, L)
    ggsw = eng.encrypt_ggsw(W, beta, L, 32, id0=0)
    eng.profile(True)
    out = eng.linear_ggsw(ggsw, beta, L, docs8, B, D, 0)
    eng.profile(False)
    assert eng.kernel_name("linear_ggsw") == "k_keyswitch_mfma<8, 1>"
    prof = eng.profile_read("linear_ggsw")
    assert prof["items"] == B
    print(f"linear_ggsw ({beta},{L}) B={B}: {prof['total_ms']:.3f} ms")
    ph = u64(eng.phase(out))
    with np.errstate(over="ignore"):
        err = (ph - ((dq @ W).astype(U) << U(64 - 16))).view(np.int64).astype(np.float64)
    sigma = float(np.sqrt(np.mean(err ** 2)))   # RMS: a bias would count too
    sigma_model = math.sqrt(extprod_var(prm, w2, beta, L))
    r = float(W.sum()) ** 2 / w2
    print(f"extprod ({beta},{L}) ||W||^2 = 2^{math.log2(w2):.2f}, (sum W)^2 / ||W||^2 = {r:.3f}: "
          f"sigma 2^{math.log2(sigma):.2f}, model 2^{math.log2(sigma_model):.2f}, ratio {sigma / sigma_model:.3f}, "
          f"max |err| {np.abs(err).max() / sigma_model:.2f} model sigmas")
    assert sigma <= 1.1 * sigma_model
    eng.close()


def test_integration_binding_ggsw(need_gpu):
    """integration/fhe_gpu.py's both-private calls (numpy and ctypes only) on
    TOY at 12 bits with planned gadgets: compare_ggsw returns the clear sums
    and bits, and search_ggsw's packed reply decrypts to the same."""
    import sys
    from pathlib import Path
    from fheicp import LIB_PATH
    from fheicp.params import extprod_var, pack_plan
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "integration"))
    from fhe_gpu import GpuCompare
    p = TOY.with_msg_bits(12)
    eng = GpuCompare(p.as_dict(), key_seed=31, lib_path=str(LIB_PATH), enc_seed=1)
    try:
        rng = np.random.default_rng(9)
        B, D = 70, 5                                     # S = 51 per GLWE: two GLWEs
        dq, W = rng.integers(-8, 8, (B, D)), rng.integers(-9, 10, D)
        cst, T = 11, -20
        want = dq @ W + cst                              # |acc - T| <= 5 * 8 * 9 + 31 < 2^11
        w2 = 0.5 * (float(np.sum(W * W)) + float(np.abs(W).sum()) ** 2)
        beta, L = eng.ggsw_plan(w2)
        assert (beta, L) == extprod_plan(p, w2)
        b, lv, lb = eng.keygen_pack(count=B, in_var=extprod_var(p, w2, beta, L) / 2.0 ** 128, seed=32)
        assert (b, lv, lb) == pack_plan(p, B, extprod_var(p, w2, beta, L) / 2.0 ** 128)
        glwe = eng.encrypt_docs_glwe(dq)
        assert glwe.size == 2 * (p.k + 1) * p.N
        ggsw = eng.encrypt_ggsw(W, beta, L)
        docs = eng.pack_docs_glwe(glwe, B, D, beta, L)
        acc1, below1 = eng.compare_ggsw(ggsw, beta, L, docs, cst, T)
        ga, gb = eng.search_ggsw(ggsw, beta, L, docs, cst, T, lb)
        acc = eng.decrypt_packed(ga, B, 0) + T
        below = eng.decrypt_packed(gb, B, 1)
        eng.free_docs(docs)
    finally:
        eng.close()
    np.testing.assert_array_equal(acc1, want)
    np.testing.assert_array_equal(acc, want)
    np.testing.assert_array_equal(below, (want < T).astype(np.int64))
    np.testing.assert_array_equal(below1, below)
    assert 0 < below.sum() < B
