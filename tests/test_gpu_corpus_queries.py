"""GPU: stored-ciphertext search for several clear queries in one batched call
and with two parties.

On TOY (dim 512: 64 of the 256 threads own a mask block) the leveled step for
Q weight rows is word for word the oracle's linear combination of the
expanded corpus and Q calls of the single-query entry, on query counts that
put a full, a short and a one-past tile on every tile size, with stream ids
that wrap 2^64 and carry into the nonce's high word; the rows after Q * B
stay untouched; an evaluation-only context answers with packed GLWEs whose
decryption equals the key holder's compare. On the real P0 = 21 parameters
compare_many, the two-party path and BatchProcessor.search_vectors equal
single calls and the clear restatement (quant_ref.corpus_*) bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import quant_ref as Q

from fheicp.engine import Engine
from fheicp.params import TOY

pytestmark = pytest.mark.gpu

U = np.uint64
SENTINEL = 0x5EA15EA15EA15EA1
# every Q in {1, 2, 3, 4, 5, 8, 9, 17}, B in {1, 7, 64}, D in {1, 3, 16, 65} in at least two shapes
SHAPES = [(1, 1, 1), (1, 7, 16), (2, 64, 3), (2, 1, 65), (3, 7, 65), (3, 64, 1), (4, 1, 16), (4, 7, 3), (5, 64, 16),
          (5, 7, 1), (8, 1, 3), (8, 64, 65), (9, 7, 16), (9, 64, 3), (17, 7, 65), (17, 1, 1)]


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def host_u64(t):
    return t.cpu().numpy().view(U)


@pytest.fixture(scope="module")
def toy(need_gpu, oracle_lib):
    eng = Engine(TOY, 0)
    eng.keygen(99)
    return eng, oracle_lib.RefTFHE(TOY.as_dict(), 99), oracle_lib


_LINEAR = {}


def run_linear(toy, Qn, B, D):
    """One batched leveled step into a buffer with 16 sentinel rows after row
    Q * B, computed once per shape: (inputs, the whole buffer)."""
    key = (Qn, B, D)
    if key not in _LINEAR:
        eng, _, ol = toy
        rng = np.random.default_rng(Qn * 100003 + B * 1009 + D)
        mk = ol.key_from_seed(11)
        body = rng.integers(0, 2 ** 64, (B, D), dtype=U)
        ids = rng.integers(0, 2 ** 64, B, dtype=U)
        if B >= 2:
            ids[0] = U(2 ** 64 - 2)       # feature ids wrap modulo 2^64 (from D = 3 on)
            ids[1] = U(2 ** 32 - 1)       # feature ids carry into the nonce's high word
        else:
            ids[0] = U(2 ** 64 - 2) if Qn % 2 else U(2 ** 32 - 1)
        W = rng.integers(-(2 ** 63), 2 ** 63, (Qn, D), dtype=np.int64)
        W[0, D // 2] = 0
        W[0, 0] = -(2 ** 63)
        W[0, D - 1] = 2 ** 63 - 1
        if Qn >= 3:
            W[1] = 0                      # an all-zero row
        if Qn >= 2:
            W[Qn - 1] = W[0]              # one query at two positions of the batch
        cst = [-37 + 11 * q for q in range(Qn)]                      # distinct per query
        buf = torch.full((Qn * B + 16, eng.W), np.array(SENTINEL, U).view(np.int64).item(), dtype=torch.int64,
                         device=eng.device)
        bd, idd = dev_u64(eng, body), dev_u64(eng, ids)
        eng.linear_seeded_queries(bd, idd, mk, W, cst, out=buf)
        _LINEAR[key] = ((body, ids, mk, W, cst, bd, idd), host_u64(buf).copy())
    return _LINEAR[key]


@pytest.mark.parametrize("Qn,B,D", SHAPES)
def test_linear_seeded_queries_bit_exact(toy, Qn, B, D):
    eng, ref, _ = toy
    P, Wd = eng.msg_bits, eng.W
    assert Wd == 513
    (body, ids, mk, W, cst, bd, idd), buf = run_linear(toy, Qn, B, D)
    got = buf[:Qn * B].reshape(Qn, B, Wd)
    ct_ref = ref.expand_seeded(body, ids, mk)
    for q in range(Qn):
        want = ref.linear(ct_ref, B, D, W[q], cst[q])
        np.testing.assert_array_equal(got[q], want, err_msg=f"query {q} against the oracle")
        one = eng.linear_seeded(bd, idd, mk, W[q], cst[q])
        np.testing.assert_array_equal(got[q], host_u64(one), err_msg=f"query {q} against the single-query entry")
    if Qn >= 3:
        assert not got[1][:, :Wd - 1].any()                          # the all-zero row: a trivial ciphertext
    if Qn >= 2:
        # the repeated query: equal masks, bodies that differ by the constant only
        np.testing.assert_array_equal(got[Qn - 1][:, :Wd - 1], got[0][:, :Wd - 1])
        with np.errstate(over="ignore"):
            delta = U((cst[Qn - 1] - cst[0]) % 2 ** 64) << U(64 - P)
            np.testing.assert_array_equal(got[Qn - 1][:, Wd - 1], got[0][:, Wd - 1] + delta)


@pytest.mark.parametrize("Qn,B,D", SHAPES)
def test_linear_seeded_queries_canary(toy, Qn, B, D):
    """The 16 rows after row Q * B keep their sentinel (the rows of a tail
    tile past Q are not stored) and every real row is overwritten."""
    _, buf = run_linear(toy, Qn, B, D)
    assert buf.shape[0] == Qn * B + 16
    assert (buf[Qn * B:] == U(SENTINEL)).all()
    assert not (buf[:Qn * B] == U(SENTINEL)).any(axis=1).any()


def test_q1_equals_linear_seeded(toy):
    eng, _, _ = toy
    for B, D in ((1, 1), (7, 16)):
        (_, _, mk, W, cst, bd, idd), buf = run_linear(toy, 1, B, D)
        one = eng.linear_seeded(bd, idd, mk, W[0], cst[0])
        np.testing.assert_array_equal(buf[:B], host_u64(one))


def test_seeded_queries_reject_bad_arguments(toy):
    eng, _, _ = toy
    L, key = eng._L, eng._key(np.arange(8, dtype=np.uint32))
    x = torch.zeros(2 * 4 * 513, dtype=torch.int64, device=eng.device)
    p = C.c_void_p(x.data_ptr())
    hv = (C.c_int64 * 4)()
    for Qn, B, D in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (65536, 2, 4), (2, 2 ** 27, 32)):
        assert L.fhe_linear_seeded_queries_batch(eng._ctx, p, p, B, D, key, Qn, p, hv, p, None) == -1
        assert b"seeded queries" in L.fhe_last_error(eng._ctx)
        assert L.fhe_compare_seeded_queries_batch(eng._ctx, p, p, B, D, key, Qn, p, 0, hv, p, p, None) == -1
        assert L.fhe_search_seeded_queries_batch(eng._ctx, p, p, B, D, key, Qn, p, 0, hv, 0, p, p, None) == -1
    assert L.fhe_linear_seeded_queries_batch(eng._ctx, p, p, 2, 4, key, 2, None, hv, p, None) == -1     # null d_W
    assert L.fhe_linear_seeded_queries_batch(eng._ctx, p, p, 2, 4, key, 2, p, None, p, None) == -1      # null h_cst
    assert L.fhe_compare_seeded_queries_batch(eng._ctx, p, p, 2, 4, key, 2, p, 0, None, p, p, None) == -1  # null h_T
    assert L.fhe_compare_seeded_queries_batch(eng._ctx, p, p, 2, 4, None, 2, p, 0, hv, p, p, None) == -1   # null key
    assert b"seeded queries" in L.fhe_last_error(eng._ctx)
    # no packing key on this context: FHE_E_STATE, as fhe_search_queries_batch
    assert L.fhe_search_seeded_queries_batch(eng._ctx, p, p, 2, 4, key, 2, p, 0, hv, 0, p, p, None) == -3


# ------------------------------------------------------- evaluation-only --
def test_search_on_evaluation_only_context(need_gpu):
    """TOY with the packing gadget (4, 3), at msg_bits = 5: the packing rounds
    the masks to 12 bits, sigma = sqrt(257 / 12) 2^52 = 2^54.2, so the half
    step 2^58 of 5-bit values stands at 13.8 sigma (at TOY's 8 bits it would
    be 1.7) and a bit's margin 2^62 far beyond. Values: D = 5, documents in
    [-2, 1], weights in [-1, 1], cst = 1, thresholds in [-2, 2] chosen on the
    clear scores so that both outcomes occur: |acc - T| <= 10 + 1 + 2 < 2^4."""
    P = 5
    A = Engine(TOY, 0)
    A.keygen(1234)
    A.keygen_pack(4, 3, seed=77)
    S = Engine(TOY, 0)
    S.import_eval_keys(A.export_eval_keys())
    A.set_msg_bits(P)
    S.set_msg_bits(P)
    mk, nk = np.arange(8, dtype=np.uint32) + 5, np.arange(8, dtype=np.uint32) + 77
    L = S._L
    n1 = (TOY.k + 1) * TOY.N
    for Qn, B, Ts in ((3, 100, [2, 1, -2]), (2, 7, [1, -1])):
        rng = np.random.default_rng(Qn * 1000 + B)
        D = 5
        dq = rng.integers(-2, 2, (B, D))
        W = rng.integers(-1, 2, (Qn, D))
        cst = 1
        want = (dq @ W.T).T + cst
        want_below = (want < np.array(Ts)[:, None]).astype(np.int64)
        ids = rng.integers(0, 2 ** 64, B, dtype=U)
        body = A.encrypt_seeded(A.to_dev(dq), mk, nk, dev_u64(A, ids))
        acc1, below1 = A.compare_seeded_queries(body, dev_u64(A, ids), mk, A.to_dev(W), cst, Ts)
        np.testing.assert_array_equal(acc1.cpu().numpy(), want)
        np.testing.assert_array_equal(below1.cpu().numpy(), want_below)
        if B == 100:
            assert all(0 < want_below[q].sum() < B for q in range(Qn))
        # the host: the same bodies and ids on its own context
        sb, si, sW = dev_u64(S, host_u64(body)), dev_u64(S, ids), S.to_dev(W)
        ga, gb = S.search_seeded_queries(sb, si, mk, sW, cst, Ts)
        G = -(-(Qn * B) // TOY.N)
        assert G == (2 if B == 100 else 1) and tuple(ga.shape) == tuple(gb.shape) == (G, n1)
        acc = A.decrypt_packed(dev_u64(A, host_u64(ga)), Qn * B, 0).reshape(Qn, B).cpu().numpy() + \
            np.array(Ts)[:, None]
        below = A.decrypt_packed(dev_u64(A, host_u64(gb)), Qn * B, 1).reshape(Qn, B).cpu().numpy()
        np.testing.assert_array_equal(acc, acc1.cpu().numpy())
        np.testing.assert_array_equal(below, below1.cpu().numpy())
        # and it can neither compare nor decrypt
        hT = (C.c_int64 * Qn)(*Ts)
        key = S._key(mk)
        out = torch.zeros((2, Qn * B), dtype=torch.int64, device=S.device)
        po = C.c_void_p(out.data_ptr())
        assert L.fhe_compare_seeded_queries_batch(S._ctx, C.c_void_p(sb.data_ptr()), C.c_void_p(si.data_ptr()), B, D,
                                                  key, Qn, C.c_void_p(sW.data_ptr()), cst, hT, po, po, None) == -3
        ct = S.empty_big(1)
        assert L.fhe_decrypt_batch(S._ctx, C.c_void_p(ct.data_ptr()), 1, po, None) == -3
    A.close()
    S.close()


# ------------------------------------------------------- real parameters --
@pytest.fixture(scope="module")
def corpus16(need_gpu, tmp_path_factory):
    """The 16-dim n_bits = 6 model of tests/test_gpu_corpus.py (P0 = 21), its
    client and a server built from evaluation keys saved and reloaded; the
    130 documents of seed 21 encrypted once; the eight queries and their
    reference accumulators."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.query import load_eval_keys, save_eval_keys
    from fheicp.stored import CorpusClient, CorpusServer
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    assert c.P0 == 21
    client = CorpusClient(c, pack_seed=17)
    assert client.margin >= 9.2
    path = str(tmp_path_factory.mktemp("keys") / "eval.npz")
    save_eval_keys(path, client.eval_keys())
    keys = load_eval_keys(path)
    server = CorpusServer(keys, cq, c.P0, c.mask_key)
    q21, docs = Q.make_corpus(16, 130, seed=21)
    queries = [q21] + [Q.make_corpus(16, 130, seed=s)[0] for s in (31, 32, 33, 34)]
    queries += [np.full(16, -10.0, np.float32), (0.05 * q21).astype(np.float32), np.zeros(16, np.float32)]
    queries = np.stack(queries)
    bodies, ids = client.encrypt_docs(docs)
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 6, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    med = [float(np.median(s)) for s in scores]
    assert [int((scores[q] < med[q]).sum()) for q in range(8)] == [65] * 7 + [0]
    assert server.load(bodies, ids) == 130
    return {"c": c, "client": client, "server": server, "queries": queries, "bodies": bodies, "ids": ids, "ref": ref,
            "scores": scores, "med": med}


BATCHES = {"all8": (list(range(8)), 21), "without-10": ([0, 1, 2, 3, 4, 6, 7], 20)}


def wanted(f, idx, ts):
    tl = ts if isinstance(ts, list) else [ts] * len(idx)
    below = np.stack([(f["scores"][q] < t).astype(np.int64) for q, t in zip(idx, tl)])
    return f["ref"][idx], below


@pytest.mark.parametrize("batch", list(BATCHES))
def test_compare_many_equals_single_and_restatement(corpus16, batch):
    f = corpus16
    c, eng = f["c"], f["c"].engine
    idx, wantP = BATCHES[batch]
    bd, idd = dev_u64(eng, f["bodies"]), dev_u64(eng, f["ids"])
    for ts in (0.5, [f["med"][q] for q in idx]):
        ref, want_below = wanted(f, idx, ts)
        acc, below, P = c.compare_many(bd, idd, f["queries"][idx], ts)
        assert P == wantP and acc.shape == below.shape == (len(idx), 130) and acc.dtype == below.dtype == torch.int64
        np.testing.assert_array_equal(acc.cpu().numpy(), ref)
        np.testing.assert_array_equal(below.cpu().numpy(), want_below)
        tl = ts if isinstance(ts, list) else [ts] * len(idx)
        for i, q in enumerate(idx):
            a1, b1, _ = c.compare(bd, idd, f["queries"][q], tl[i])
            assert torch.equal(a1, acc[i]) and torch.equal(b1, below[i]), q
        if isinstance(ts, list):
            # both sides of the sign extraction for every non-degenerate query
            got = below.cpu().numpy()
            for i, q in enumerate(idx):
                if q != 7:
                    assert 0.4 <= got[i].mean() <= 0.6, q
                else:
                    assert got[i].sum() == 0


@pytest.mark.parametrize("batch", list(BATCHES))
def test_two_party_search_many(corpus16, batch):
    f = corpus16
    client, server = f["client"], f["server"]
    idx, wantP = BATCHES[batch]
    n1 = (f["c"].scheme.k + 1) * f["c"].scheme.N
    for ts in (0.5, [f["med"][q] for q in idx]):
        ref, want_below = wanted(f, idx, ts)
        replies = server.search_many(f["queries"][idx], ts)
        G = -(-(len(idx) * 130) // f["c"].scheme.N)
        assert isinstance(replies, list) and len(replies) == 1
        assert replies[0].dtype == U and replies[0].size == 4 + len(idx) + 2 * G * n1
        assert int(replies[0][1]) == 2 | (wantP << 32)               # the width field carries the chunk's P
        acc, below = client.decrypt_replies(replies)
        np.testing.assert_array_equal(acc.cpu().numpy(), ref)
        np.testing.assert_array_equal(below.cpu().numpy(), want_below)
    # one query: the single-element case
    one = server.search(f["queries"][0], 0.5)
    acc, below = client.decrypt_replies(one)
    ref, want_below = wanted(f, [0], 0.5)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(below.cpu().numpy(), want_below)
    from fheicp import _lib
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        server.engine.decrypt(server.engine.empty_big(1))
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        server.engine.compare_seeded_queries(server.body, server.ids, server.mask_key,
                                             server.engine.to_dev(np.zeros((1, 16), np.int64)), 0, [0])


def test_batch_processor_search_vectors_ciphertext_store(tmp_path, need_gpu, monkeypatch):
    from batch_operations import BatchConfig, BatchProcessor
    monkeypatch.setenv("FHE_MASTER_PASSWORD", "corpus-pw")
    from encrypted_storage import EncryptedDocumentStore
    cfg = BatchConfig(input_dim=16, n_bits=6, seed=3, key_seed=8, store_ciphertexts=True,
                      corpus_path=str(tmp_path / "corpus.npz"), batch_size=100, key_manager_default=False)
    bp = BatchProcessor(storage=EncryptedDocumentStore(str(tmp_path / "docs")), config=cfg)
    q0, docs = Q.make_corpus(16, 300, seed=23)
    names = [f"doc{i:04d}" for i in range(len(docs))]
    bp.store_vectors(docs, names)
    queries = [q0, Q.make_corpus(16, 1, seed=24)[0], docs[5], np.full(16, -10.0, np.float32), np.zeros(16, np.float32)]
    calls = []
    c = bp.corpus_engine
    orig = c.compare_many
    c.compare_many = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    got = bp.search_vectors(queries, top_k=10, min_similarity=0.5)
    assert calls == [1]                                  # the batched path: one compare_many for the resident corpus
    want = [bp.search_vector(q, top_k=10, min_similarity=0.5) for q in queries]
    assert got == want                                   # same ids, same order, scores equal as floats
    oq = Q.QuantizedLinearParams.from_json(bp.fhe_model.model.quant_params.to_dict())
    for q, g in zip(queries, got):
        assert g == [(names[i], s) for i, s in Q.corpus_search(oq, c.cq.s_e, c.cq.n_e, q, docs, 10, 0.5)]
    assert len(got) == 5 and len(got[0]) > 0
    assert bp.search_vectors([], top_k=10) == []
