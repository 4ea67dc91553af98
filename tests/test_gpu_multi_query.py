"""GPU: several private queries in one batched call.

The leveled step for Q queries is word for word the plain u64 sum and Q calls
of the single-query entry, on shapes with partial document groups and query
row offsets that are no multiple of 16, and leaves the rows after Q * B alone.
End to end, every decrypted accumulator and threshold bit of compare_many and
of search_many -> decrypt_replies (an evaluation-only server) equals Q single
calls and the clear restatement (quant_ref.corpus_*), on TOY (n = 64, N = 256,
W = 513: the last column block holds one real column) and once on the real
P0 = 21 parameters; BatchProcessor.search_vectors equals the list of
search_vector results."""
import numpy as np
import pytest
import torch

from oracle import quant_ref as Q

from fheicp.engine import Engine
from fheicp.params import TOY

pytestmark = pytest.mark.gpu

U = np.uint64
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF)
SENTINEL = 0x5EA15EA15EA15EA1
# every Q, B and D of the issue's axes in at least two shapes
SHAPES = [(1, 1, 1), (2, 15, 16), (3, 17, 65), (5, 130, 130), (2, 16, 130), (1, 33, 65), (5, 1, 16), (3, 15, 1),
          (2, 17, 16), (3, 33, 130), (2, 130, 1), (5, 16, 65)]


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def host_u64(t):
    return t.cpu().numpy().view(U)


@pytest.fixture(scope="module")
def toy(need_gpu):
    eng = Engine(TOY, 0)
    eng.keygen(99)
    return eng


_LINEAR = {}


def run_linear(eng, Qn, B, D):
    """One batched leveled step into a buffer with 16 sentinel rows after
    row Q * B, computed once per shape: (inputs, the whole buffer)."""
    key = (Qn, B, D)
    if key not in _LINEAR:
        W = eng.W
        rng = np.random.default_rng(Qn * 100003 + B * 1009 + D)
        ct = rng.integers(0, 2 ** 64, (Qn, D, W), dtype=U)
        for r, word in zip((0, D // 2, D - 1), EDGE_WORDS):
            ct[0, r, :] = U(word)
        if Qn >= 2:
            ct[Qn - 1] = ct[0]            # one query at two positions of the batch
        dq = rng.integers(-128, 128, (B, D))
        dq[0, :] = -128
        dq[B - 1, :] = 127
        w = rng.integers(-(2 ** 63), 2 ** 63, D, dtype=np.int64)
        w[0] = -(2 ** 63)
        w[D - 1] = 2 ** 63 - 1
        cst = [-37 + 11 * q for q in range(Qn)]                      # distinct per query
        docs8 = eng.pack_docs(eng.to_dev(dq))
        buf = torch.full((Qn * B + 16, W), np.array(SENTINEL, U).view(np.int64).item(), dtype=torch.int64,
                         device=eng.device)
        eng.linear_queries(dev_u64(eng, ct.reshape(Qn * D, W)), Qn, docs8, B, D, w, cst, out=buf)
        _LINEAR[key] = ((ct, dq, w, cst, docs8), host_u64(buf).copy())
    return _LINEAR[key]


@pytest.mark.parametrize("Qn,B,D", SHAPES)
def test_linear_queries_bit_exact(toy, Qn, B, D):
    eng = toy
    P, W = eng.msg_bits, eng.W
    assert W == 513
    (ct, dq, w, cst, docs8), buf = run_linear(eng, Qn, B, D)
    got = buf[:Qn * B].reshape(Qn, B, W)
    for q in range(Qn):
        with np.errstate(over="ignore"):
            want = dq.astype(U) @ (w.astype(U)[:, None] * ct[q])
            want[:, W - 1] += U(cst[q] % 2 ** 64) << U(64 - P)
        np.testing.assert_array_equal(got[q], want, err_msg=f"query {q} against the u64 restatement")
        one = eng.linear_query(dev_u64(eng, ct[q]), docs8, B, D, w, cst[q])
        np.testing.assert_array_equal(got[q], host_u64(one), err_msg=f"query {q} against the single-query entry")
    if Qn >= 2:
        # the repeated query: identical row blocks but for the two constants
        np.testing.assert_array_equal(got[Qn - 1][:, :W - 1], got[0][:, :W - 1])
        with np.errstate(over="ignore"):
            delta = U((cst[Qn - 1] - cst[0]) % 2 ** 64) << U(64 - P)
            np.testing.assert_array_equal(got[Qn - 1][:, W - 1], got[0][:, W - 1] + delta)


@pytest.mark.parametrize("Qn,B,D", SHAPES)
def test_linear_queries_canary(toy, Qn, B, D):
    """The 16 rows after row Q * B keep their sentinel: the padded rows of the
    last document group of the last query are not stored."""
    _, buf = run_linear(toy, Qn, B, D)
    assert buf.shape[0] == Qn * B + 16
    assert (buf[Qn * B:] == U(SENTINEL)).all()
    assert not (buf[:Qn * B] == U(SENTINEL)).all(axis=1).any()        # and every real row was written


def test_queries_reject_bad_arguments(toy):
    import ctypes as C
    eng = toy
    L, key = eng._L, eng._key(np.arange(8, dtype=np.uint32))
    x = torch.zeros(16 * 64 * 8, dtype=torch.int64, device=eng.device)
    p = C.c_void_p(x.data_ptr())
    hc = (C.c_int64 * 4)()
    for Qn, B, D in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (2, 2, 65537)):
        assert L.fhe_linear_queries_batch(eng._ctx, p, Qn, p, B, D, p, hc, p, None) == -1
        assert b"queries" in L.fhe_last_error(eng._ctx)
        assert L.fhe_compare_queries_batch(eng._ctx, p, p, key, Qn, p, B, D, p, 0, hc, p, p, None) == -1
    assert L.fhe_linear_queries_batch(eng._ctx, p, 2, p, 2, 4, p, None, p, None) == -1        # null constants
    assert L.fhe_compare_queries_batch(eng._ctx, p, None, key, 2, p, 2, 4, p, 0, hc, p, p, None) == -1   # null ids
    assert L.fhe_compare_queries_batch(eng._ctx, p, p, None, 2, p, 2, 4, p, 0, hc, p, p, None) == -1     # null mask key
    # no packing key on this context: FHE_E_STATE, as fhe_search_query_batch
    assert L.fhe_search_queries_batch(eng._ctx, p, p, key, 2, p, 2, 4, p, 0, hc, 0, p, p, None) == -3


# ------------------------------------------------------------- end to end --
def make_inputs(rng, Qn, B, D, lo, hi):
    return rng.uniform(lo, hi, (Qn, D)).astype(np.float32), rng.uniform(lo, hi, (B, D)).astype(np.float32)


@pytest.fixture(scope="module")
def toy_corpus(need_gpu):
    """A 5-feature, 2-bit model whose worst-case width is TOY's 8 bits
    (bound = 4 * sum|q_w| + |q_b'| = 35): client on the corpus context, server
    from the evaluation keys only. Q = 3 queries, B = 130 documents."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.model import QuantParams
    from fheicp.query import EncryptedQuerySearch, QueryClient, QueryServer
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    cq = CorpusQuant(qp, 2, 0.5)
    assert cq.q_b == 3
    c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=5, device=0, noise_seed=6)
    assert c.P0 == 8 == TOY.msg_bits
    oq = Q.QuantizedLinearParams.from_json(qp.to_dict())
    single = EncryptedQuerySearch(c)
    client = QueryClient(c, count=TOY.N, pack_seed=17)
    server = QueryServer(client.eval_keys(), cq, c.P0, scheme=c.scheme)
    Qn, B = 3, 130
    qs, docs = make_inputs(np.random.default_rng(77), Qn, B, 5, -1.2, 0.7)
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 2, q, docs) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    # distinct thresholds: None (T = -bound), the median of query 1's scores
    # (both outcomes occur there), a fixed one
    ts = [None, float(np.median(scores[1])), 0.5]
    want_below = np.stack([np.zeros(B, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                           for q, t in enumerate(ts)])
    assert 0 < want_below[1].sum() < B
    assert len({single.plan(t)[2] for t in ts}) == 3
    return {"c": c, "single": single, "client": client, "server": server, "qs": qs, "docs": docs, "ref": ref,
            "ts": ts, "below": want_below, "B": B}


def test_compare_many_equals_single_and_restatement(toy_corpus):
    f = toy_corpus
    single, B = f["single"], f["B"]
    payloads = single.encrypt_queries(f["qs"])
    assert len(payloads) == 3
    for q, pl in enumerate(payloads):
        np.testing.assert_array_equal(single.decrypt_query(pl), Q.corpus_quant(single.cq.s_e, 2, f["qs"][q]))
    docs8 = single.pack_docs(f["docs"])
    acc, below = single.compare_many(payloads, docs8, B, f["ts"])
    assert acc.shape == below.shape == (3, B) and acc.dtype == below.dtype == torch.int64
    np.testing.assert_array_equal(acc.cpu().numpy(), f["ref"])
    np.testing.assert_array_equal(below.cpu().numpy(), f["below"])
    for q, pl in enumerate(payloads):
        a1, b1 = single.compare(pl, docs8, B, f["ts"][q])
        assert torch.equal(a1, acc[q]) and torch.equal(b1, below[q]), q
    # one scalar threshold for all, and a batch the server must refuse
    acc2, below2 = single.compare_many(payloads, docs8, B, f["ts"][1])
    np.testing.assert_array_equal(acc2.cpu().numpy(), f["ref"])
    scores = single.scores(f["ref"])
    np.testing.assert_array_equal(below2.cpu().numpy(), (scores < f["ts"][1]).astype(np.int64))
    with pytest.raises(ValueError, match="query 2.*overlap"):
        single.compare_many(payloads[:2] + [payloads[0]], docs8, B, None)


def test_two_party_search_many(toy_corpus):
    f = toy_corpus
    client, server, B = f["client"], f["server"], f["B"]
    p = TOY
    payloads = client.encrypt_queries(f["qs"])
    docs8 = server.pack_docs(f["docs"])
    replies = server.search_many(payloads, docs8, B, f["ts"])
    assert isinstance(replies, list) and len(replies) == 1
    # 390 results: two GLWEs per block, query 1's results straddle coefficient 256
    assert -(-3 * B // p.N) == 2 and B < p.N < 2 * B
    assert replies[0].dtype == U and replies[0].size == 4 + 3 + 2 * 2 * (p.k + 1) * p.N
    acc, below = client.decrypt_replies(replies)
    assert acc.shape == below.shape == (3, B)
    np.testing.assert_array_equal(acc.cpu().numpy(), f["ref"])
    np.testing.assert_array_equal(below.cpu().numpy(), f["below"])
    from fheicp import _lib
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*secret"):
        server.engine.decrypt(server.engine.empty_big(1))
    with pytest.raises(ValueError, match="size"):
        client.decrypt_replies([replies[0][:-2 * (p.k + 1) * p.N]])


def test_reference_side_binding_queries(need_gpu):
    """integration/fhe_gpu.py's batched calls (numpy and ctypes only), on TOY
    at 12 bits as tests/test_gpu_pack.py's single-query binding test: 3
    queries x 100 documents, 300 results in two GLWEs."""
    import sys
    from pathlib import Path
    from fheicp import LIB_PATH
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "integration"))
    from fhe_gpu import GpuCompare
    p = TOY.with_msg_bits(12)
    eng = GpuCompare(p.as_dict(), key_seed=31, lib_path=str(LIB_PATH), enc_seed=1)
    try:
        _, _, lb = eng.keygen_pack(count=256, seed=32)
        rng = np.random.default_rng(10)
        Qn, B, D = 3, 100, 5
        dq, qq, w = rng.integers(-8, 8, (B, D)), rng.integers(-8, 8, (Qn, D)), rng.integers(-3, 4, D)
        cst, Ts = 11, [-20, 0, 35]
        want = (dq @ (w * qq).T).T + cst                 # |acc - T| <= 5 * 8 * 8 * 3 + 46 < 2^11
        docs = eng.pack_docs(dq)
        mk, nk = np.arange(8, dtype=np.uint32) + 5, np.arange(8, dtype=np.uint32) + 77
        enc = [eng.encrypt_query(qq[q], mk, nk, id0=1000 + q * D) for q in range(Qn)]
        bodies, ids = np.stack([b for b, _ in enc]), [i for _, i in enc]
        acc1, below1 = eng.compare_queries(bodies, ids, mk, docs, w, cst, Ts)
        ga, gb = eng.search_queries(bodies, ids, mk, docs, w, cst, Ts, lb)
        assert ga.size == gb.size == 2 * (p.k + 1) * p.N
        acc = eng.decrypt_packed(ga, Qn * B, 0).reshape(Qn, B) + np.array(Ts)[:, None]
        below = eng.decrypt_packed(gb, Qn * B, 1).reshape(Qn, B)
        eng.free_docs(docs)
    finally:
        eng.close()
    np.testing.assert_array_equal(acc1, want)
    np.testing.assert_array_equal(acc, want)
    np.testing.assert_array_equal(below, (want < np.array(Ts)[:, None]).astype(np.int64))
    np.testing.assert_array_equal(below1, below)
    assert all(0 < below[q].sum() < B for q in range(Qn))


@pytest.fixture(scope="module")
def real_two_party(need_gpu):
    """The 16-dim, n_bits 6 model of tests/test_gpu_pack.py (P0 = 21)."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.query import EncryptedQuerySearch, QueryClient, QueryServer
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    assert c.P0 == 21
    client = QueryClient(c, pack_seed=17)
    return c, EncryptedQuerySearch(c), client, QueryServer(client.eval_keys(), cq, c.P0), oq


def test_real_parameters_q4_b64(real_two_party):
    c, single, client, server, oq = real_two_party
    s_e = c.cq.s_e
    Qn, B = 4, 64
    qs = []
    for i in range(Qn):
        q, docs_i = Q.make_corpus(16, B, seed=40 + i)
        qs.append(q)
        if i == 0:
            docs = docs_i
    ref = np.stack([Q.corpus_accumulate(oq, s_e, 6, q, docs) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, s_e)) * ref.astype(np.float64)
    ts = [0.5, float(np.median(scores[1])), None, float(np.median(scores[3]))]
    want = np.stack([np.zeros(B, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                     for q, t in enumerate(ts)])
    assert 0.25 <= want[1].mean() <= 0.75
    payloads = client.encrypt_queries(np.stack(qs))
    acc, below = single.compare_many(payloads, single.pack_docs(docs), B, ts)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(below.cpu().numpy(), want)
    replies = server.search_many(payloads, server.pack_docs(docs), B, ts)
    n1 = (c.scheme.k + 1) * c.scheme.N
    assert len(replies) == 1 and replies[0].size == 4 + Qn + 2 * n1          # 256 results: one GLWE per block
    acc2, below2 = client.decrypt_replies(replies)
    np.testing.assert_array_equal(acc2.cpu().numpy(), ref)
    np.testing.assert_array_equal(below2.cpu().numpy(), want)


def test_batch_processor_search_vectors(tmp_path, need_gpu, monkeypatch):
    from batch_operations import BatchConfig, BatchProcessor
    monkeypatch.setenv("FHE_MASTER_PASSWORD", "query-pw")
    from encrypted_storage import EncryptedDocumentStore
    cfg = BatchConfig(input_dim=16, n_bits=6, seed=3, key_seed=8, encrypt_query=True,
                      corpus_path=str(tmp_path / "corpus.npz"), batch_size=64, key_manager_default=False)
    bp = BatchProcessor(storage=EncryptedDocumentStore(str(tmp_path / "docs")), config=cfg)
    q0, docs = Q.make_corpus(16, 150, seed=23)                               # document chunks of 64, 64, 22
    bp.store_vectors(docs, [f"doc{i:04d}" for i in range(len(docs))])
    queries = [q0, Q.make_corpus(16, 1, seed=24)[0], docs[5]]
    got = bp.search_vectors(queries, top_k=10, min_similarity=0.5)
    want = [bp.search_vector(q, top_k=10, min_similarity=0.5) for q in queries]
    assert got == want                                   # same ids, same order, scores equal as floats
    assert len(got) == 3 and len(got[0]) > 0
    assert bp.search_vectors([], top_k=10) == []
