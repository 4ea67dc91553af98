"""GPU: the private-query mode through libfheicp.

The leveled step (document packing, query byte planes, the i8 MFMA GEMM) is
bit-identical modulo 2^64 to the plain u64 sum; end to end, every decrypted
accumulator and threshold bit of fhe_compare_query_batch equals the oracle's
restatement (quant_ref.corpus_*) and the stored-ciphertext mode's, and a
BatchProcessor with encrypt_query returns the oracle's top-k."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import quant_ref as Q

from fheicp.engine import Engine
from fheicp.params import TOY, params_for_bits

pytestmark = pytest.mark.gpu

EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF)


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(eng.device)


@pytest.fixture(scope="module")
def engines(need_gpu):
    out = {}
    for name, p in (("toy", TOY), ("p16", params_for_bits(16))):
        eng = Engine(p, 0)
        eng.keygen(99)
        out[name] = eng
    return out


@pytest.mark.parametrize("which,B,D", [("toy", 1, 1), ("toy", 17, 3), ("toy", 16, 64), ("toy", 33, 65),
                                       ("toy", 130, 130), ("p16", 40, 16), ("p16", 20, 768)])
def test_linear_query_bit_exact(engines, which, B, D):
    eng = engines[which]
    P = eng.msg_bits
    W = eng.W
    assert W == (513 if which == "toy" else 2049)   # a partial last column block
    rng = np.random.default_rng(B * 1009 + D)
    ct = eng.encrypt(rng.integers(-4, 4, D), seed=B + D, id0=7).cpu().numpy().view(np.uint64).reshape(D, W).copy()
    for r, word in zip((0, D // 2, D - 1), EDGE_WORDS):
        ct[r, :] = np.uint64(word)
    dq = rng.integers(-128, 128, (B, D))
    dq[0, :] = -128
    dq[B - 1, :] = 127
    w = rng.integers(-(2 ** 63), 2 ** 63, D, dtype=np.int64)
    cst = -37
    docs8 = eng.pack_docs(eng.to_dev(dq))
    assert docs8.numel() == -(-B // 16) * 16 * -(-D // 64) * 64
    out = eng.linear_query(dev_u64(eng, ct), docs8, B, D, w, cst)
    with np.errstate(over="ignore"):
        # the u64 sum_j dq[b, j] * (w[j] * ct[j]), as one integer matrix product
        want = dq.astype(np.uint64) @ (w.astype(np.uint64)[:, None] * ct)
        want[:, W - 1] += np.uint64(cst % 2 ** 64) << np.uint64(64 - P)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), want)

    # small weights and clean ciphertexts: the result decrypts to the clear
    # dot product (|value| <= 768 * 128 * 6 < 2^23; noise <= 2^(17 + 19) << 2^39)
    eng.set_msg_bits(24)
    try:
        m = rng.integers(-2, 3, D)
        ws = rng.integers(-3, 4, D)
        ct2 = eng.encrypt(m, seed=3 * B + D, id0=11)
        out2 = eng.linear_query(ct2, docs8, B, D, ws, cst)
        np.testing.assert_array_equal(eng.decrypt(out2).cpu().numpy(), dq @ (ws * m) + cst)
    finally:
        eng.set_msg_bits(P)


def test_query_rejects_bad_arguments(engines):
    eng = engines["toy"]
    L, key = eng._L, eng._key(np.arange(8, dtype=np.uint32))
    x = torch.zeros(16 * 64 * 8, dtype=torch.int64, device=eng.device)
    p = C.c_void_p(x.data_ptr())
    assert L.fhe_query_docs_pack(eng._ctx, p, 2, 0, p, None) == -1                       # D = 0
    assert b"query" in L.fhe_last_error(eng._ctx)
    assert L.fhe_query_docs_pack(eng._ctx, p, 2, 65537, p, None) == -1                   # D > 65536
    assert L.fhe_query_docs_pack(eng._ctx, p, -1, 4, p, None) == -1                      # B < 0
    assert L.fhe_query_docs_pack(eng._ctx, None, 2, 4, p, None) == -1                    # null documents
    assert b"query" in L.fhe_last_error(eng._ctx)
    assert L.fhe_linear_query_batch(eng._ctx, p, p, 2, 65537, p, 0, p, None) == -1
    assert b"query" in L.fhe_last_error(eng._ctx)
    assert L.fhe_linear_query_batch(eng._ctx, p, p, -1, 4, p, 0, p, None) == -1
    assert L.fhe_linear_query_batch(eng._ctx, p, None, 2, 4, p, 0, p, None) == -1        # null packed documents
    assert b"query" in L.fhe_last_error(eng._ctx)
    assert L.fhe_compare_query_batch(eng._ctx, p, 0, key, p, 2, 0, p, 0, 0, p, p, None) == -1
    assert L.fhe_compare_query_batch(eng._ctx, p, 0, None, p, 2, 4, p, 0, 0, p, p, None) == -1   # null mask key
    assert b"query" in L.fhe_last_error(eng._ctx)
    assert L.fhe_compare_query_batch(eng._ctx, None, 0, key, p, 2, 4, p, 0, 0, p, p, None) == -1
    # empty batches
    assert L.fhe_query_docs_pack(eng._ctx, None, 0, 4, None, None) == 0
    assert L.fhe_linear_query_batch(eng._ctx, None, None, 0, 4, None, 0, None, None) == 0
    assert L.fhe_compare_query_batch(eng._ctx, None, 0, key, None, 0, 4, None, 0, 0, None, None, None) == 0


@pytest.fixture(scope="module")
def corpus16(need_gpu):
    """The 16-dim, n_bits 6 model of tests/test_gpu_corpus.py."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.query import EncryptedQuerySearch
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    return c, EncryptedQuerySearch(c), oq


def check_compare(qs, oq, q, docs, t, balanced=False):
    s_e = qs.cq.s_e
    ref_acc = Q.corpus_accumulate(oq, s_e, 6, q, docs)
    scores = np.float64(Q.corpus_out_scale(oq, s_e)) * ref_acc.astype(np.float64)
    payload = qs.encrypt_query(q)
    np.testing.assert_array_equal(qs.decrypt_query(payload), Q.corpus_quant(s_e, 6, q))
    docs8 = qs.pack_docs(docs)
    acc, below = qs.compare(payload, docs8, len(docs), t)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref_acc)
    want = (scores < t).astype(np.int64)
    np.testing.assert_array_equal(below.cpu().numpy(), want)
    if balanced:
        assert 0.25 <= want.mean() <= 0.75


def test_query_compare_bit_exact(corpus16):
    c, qs, oq = corpus16
    assert qs.P0 == c.P0 == Q.corpus_worst_bits(oq, c.cq.s_e, 6)
    q, docs = Q.make_corpus(16, 256, seed=21)
    scores = np.float64(Q.corpus_out_scale(oq, c.cq.s_e)) * \
        Q.corpus_accumulate(oq, c.cq.s_e, 6, q, docs).astype(np.float64)
    check_compare(qs, oq, q, docs, 0.5)
    check_compare(qs, oq, q, docs, float(np.median(scores)), balanced=True)
    # clipped (un-normalised) documents and the all-qmin query: the worst case P0 is sized for
    _, docs_c = Q.make_corpus(16, 128, seed=22, clip_set=True)
    q_min = np.full(16, -10.0, np.float32)
    scores_c = np.float64(Q.corpus_out_scale(oq, c.cq.s_e)) * \
        Q.corpus_accumulate(oq, c.cq.s_e, 6, q_min, docs_c).astype(np.float64)
    check_compare(qs, oq, q_min, docs_c, 0.5)
    check_compare(qs, oq, q_min, docs_c, float(np.median(scores_c)), balanced=True)


def test_query_matches_corpus_mode(corpus16):
    c, qs, oq = corpus16
    q, docs = Q.make_corpus(16, 100, seed=24)
    bodies, ids = c.encrypt_docs(docs)
    acc_c, below_c, _ = c.compare(dev_u64(c.engine, bodies), dev_u64(c.engine, ids), q, 0.5)
    acc_q, below_q = qs.compare(qs.encrypt_query(q), qs.pack_docs(docs), len(docs), 0.5)
    np.testing.assert_array_equal(acc_q.cpu().numpy(), acc_c.cpu().numpy())
    np.testing.assert_array_equal(below_q.cpu().numpy(), below_c.cpu().numpy())


def test_batch_processor_private_query(tmp_path, need_gpu, monkeypatch):
    from batch_operations import BatchConfig, BatchProcessor
    monkeypatch.setenv("FHE_MASTER_PASSWORD", "query-pw")   # wraps the corpus file's secret keys
    from encrypted_storage import EncryptedDocumentStore
    cfg = BatchConfig(input_dim=16, n_bits=6, seed=3, key_seed=8, encrypt_query=True,
                      corpus_path=str(tmp_path / "corpus.npz"), batch_size=100, key_manager_default=False)
    store = EncryptedDocumentStore(str(tmp_path / "docs"))
    bp = BatchProcessor(storage=store, config=cfg)
    q, docs = Q.make_corpus(16, 300, seed=23)
    names = [f"doc{i:04d}" for i in range(len(docs))]
    bp.store_vectors(docs, names)
    assert store.load("doc0007").model_version == "1.0"      # the store stays plaintext, as the reference's
    c = bp.corpus_engine
    oq = Q.QuantizedLinearParams.from_json(bp.fhe_model.model.quant_params.to_dict())
    want = Q.corpus_search(oq, c.cq.s_e, c.cq.n_e, q, docs, 10, 0.5)
    got = bp.search_vector(q, top_k=10, min_similarity=0.5)
    assert got == [(names[i], s) for i, s in want]
    assert len(got) > 0
    # a new process: keys + mask key from corpus_path, documents from disk
    bp2 = BatchProcessor(storage=EncryptedDocumentStore(str(tmp_path / "docs")), config=cfg)
    assert bp2.search_vector(q, top_k=10, min_similarity=0.5) == got
