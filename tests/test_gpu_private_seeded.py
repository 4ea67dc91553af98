"""GPU: the both-private search on seeded payloads through
libfheicp.

The expansion of seeded documents and queries word for word against the
full-form encryption under one key and against the numpy restatement
(tests/seeded_private_ref.py); the document operands made straight from the
bodies byte for byte against the full-form packers; the leveled step against
tests/extprod_ref.py; the evaluation-only server end to end on the 16-dim
model, word for word against full-form payloads of the same words; a hub with
one seeded and one full-form tenant; the integration binding. Shapes are
tests/test_gpu_private_queries.py's: the smallest that cross a 16-row tile,
leave the last GLWE partly filled and give a thread one ChaCha block."""
import ctypes as C

import numpy as np
import pytest
import torch

import extprod_ref as X
import seeded_private_ref as S
from oracle import quant_ref as Q
from oracle import tfhe_ref

from fheicp import _lib
from fheicp.engine import Engine, u64
from fheicp.params import TOY

pytestmark = pytest.mark.gpu

U = np.uint64
GADGETS = [(4, 3), (7, 7)]
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0, 1 << 63)   # tests/test_gpu_extprod.py's
DOC_ID0 = 2 ** 64 - 3          # 17 document GLWEs: ids 2^64 - 3 .. 2^64 - 1, then 0 .. 13
QUERY_IDS = [2 ** 64 - 2, 1000, 5000, 9000, 13000, 17000]     # the first query's ids wrap


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(eng.device)


@pytest.fixture(scope="module")
def toy(need_gpu):
    tfhe_ref.build()
    eng = Engine(TOY, 0)
    eng.keygen(99)
    return eng


@pytest.fixture(scope="module")
def keys(toy):
    return {"one": toy.key_from_seed(77), "mask": toy.key_from_seed(78), "noise": toy.key_from_seed(79)}


@pytest.mark.parametrize("gadget", GADGETS)
def test_expansion_equals_full_form(toy, keys, gadget):
    """Q = 3 GGSWs and G = 17 document GLWEs. With mask key = noise key = K the
    expansion of the seeded ciphertexts is fhe_encrypt_ggsw_key /
    fhe_encrypt_packed_batch_key under K word for word (ids that wrap among
    them). With distinct keys the masks are the restatement's and the bodies
    decrypt to the inputs."""
    eng = toy
    p = eng.params
    beta, L = gadget
    K1, Km, Kn = keys["one"], keys["mask"], keys["noise"]
    rng = np.random.default_rng(10 * beta + L)
    Ws = rng.integers(-2 ** 12, 2 ** 12, (3, 16))
    ids = QUERY_IDS[:3]
    bodies = torch.stack([eng.encrypt_ggsw_seeded(w, beta, L, K1, K1, i) for w, i in zip(Ws, ids)])
    assert bodies.shape == (3, (p.k + 1) * L, p.N) and bodies[0].numel() == eng.ggsw_body_words(beta, L)
    got = u64(eng.expand_ggsws_seeded(bodies, ids, beta, L, K1))
    assert got.shape == (3, eng.ggsw_words(beta, L))
    for q, (w, i) in enumerate(zip(Ws, ids)):
        np.testing.assert_array_equal(got[q], u64(eng.encrypt_ggsw(w, beta, L, K1, i)).reshape(-1),
                                      err_msg=f"query {q} against fhe_encrypt_ggsw_key")
    D, S_ = 16, p.N // 16
    dq = rng.integers(-8, 8, (16 * S_ + 5, D))             # 17 GLWEs, the last partly filled
    assert p.msg_bits >= 5
    assert eng.doc_glwes(len(dq), D) == 17
    db = eng.encrypt_docs_glwe_seeded(dq, K1, K1, DOC_ID0)
    assert db.shape == (17, p.N)
    np.testing.assert_array_equal(u64(eng.expand_docs_glwe_seeded(db, DOC_ID0, K1)),
                                  u64(eng.encrypt_docs_glwe(dq, K1, DOC_ID0)))
    # distinct keys: public masks, secret noise
    b2 = torch.stack([eng.encrypt_ggsw_seeded(w, beta, L, Km, Kn, i) for w, i in zip(Ws, ids)])
    g2 = u64(eng.expand_ggsws_seeded(b2, ids, beta, L, Km)).reshape(3, (p.k + 1) * L, p.k + 1, p.N)
    for q, i in enumerate(ids):
        np.testing.assert_array_equal(g2[q, :, :p.k], S.ggsw_masks(Km, i, p.N, p.k, L), err_msg=f"query {q} masks")
        np.testing.assert_array_equal(g2[q, :, p.k], u64(b2[q]))
        assert not np.array_equal(g2[q, :, p.k], u64(bodies[q]))       # other masks, other noise: other bodies
    d2 = eng.encrypt_docs_glwe_seeded(dq, Km, Kn, DOC_ID0)
    e2 = eng.expand_docs_glwe_seeded(d2, DOC_ID0, Km)
    np.testing.assert_array_equal(u64(e2).reshape(17, p.k + 1, p.N), S.expand_glwe(u64(d2), Km, DOC_ID0, p.N, p.k))
    dec = eng.decrypt_packed(e2, 17 * p.N, 0).cpu().numpy().reshape(17, p.N)
    np.testing.assert_array_equal(dec[:, :S_ * D].reshape(17 * S_, D)[:len(dq)], dq)


@pytest.fixture(scope="module")
def seeded_docs(toy, keys):
    """Per gadget: 17 seeded document bodies of arbitrary words with the edge
    words and, on every level, the tie inputs with both coins, planted in the
    BODY (masks cannot be planted); their expansion by the library, checked
    against the restatement once."""
    eng = toy
    p = eng.params
    Km = keys["mask"]
    masks = S.glwe_masks(Km, DOC_ID0, 17, p.N, p.k)
    out = {}
    for beta, L in GADGETS:
        rng = np.random.default_rng(300 * beta + L)
        body = rng.integers(0, 2 ** 64, (17, p.N), dtype=U)
        for i, w in enumerate(EDGE_WORDS):
            body[i % 17, 5 * i:5 * i + 3] = U(w)
        prec = beta * L
        ties = [((1 << (beta - 1)) << (64 - beta * l)) | (c << (62 - prec - (L - l))) for l in range(1, L + 1)
                for c in (0, 1)]
        for g in (0, 1, 16):                               # in every G of the cases below
            body[g, 40:40 + len(ties)] = np.array(ties, U)
        full = u64(eng.expand_docs_glwe_seeded(dev_u64(eng, body), DOC_ID0, Km)).reshape(17, p.k + 1, p.N)
        np.testing.assert_array_equal(full[:, :p.k], masks)
        np.testing.assert_array_equal(full[:, p.k], body)
        # the regenerated words of these ids (DOC_ID0 on, under keys["mask"]) hit both digit signs on
        # every level, GLWE by GLWE, so a wrong sign or level in the mask branch cannot hide
        for g in range(17):
            neg, pos = S.digit_signs(masks[g], beta, L)
            assert neg.all() and pos.all(), (beta, L, g)
        out[(beta, L)] = (body, full)
    return out


def _shape(p, G, D):
    S_ = p.N // D
    B = G * S_ if S_ == 1 else (G - 1) * S_ + max(1, S_ // 3)   # the last GLWE partly filled
    return S_, B


DOC_CASES = [((4, 3), 1, 1), ((4, 3), 2, 5), ((4, 3), 17, 16), ((4, 3), 2, 256), ((4, 3), 17, 1),
             ((7, 7), 17, 256), ((7, 7), 1, 16), ((7, 7), 2, 1), ((7, 7), 17, 5), ((7, 7), 1, 256)]
SENT = 0xA5


@pytest.mark.parametrize("gadget,G,D", DOC_CASES)
def test_document_operands_from_bodies_byte_for_byte(toy, keys, seeded_docs, gadget, G, D):
    """fhe_glwe_docs_pack_seeded / fhe_glwe_docs_queries_pack_seeded on the
    bodies equal fhe_glwe_docs_pack / fhe_glwe_docs_queries_pack on the
    expanded GLWEs byte for byte, and 16 sentinel bytes after each operand
    stay untouched."""
    eng = toy
    p = eng.params
    beta, L = gadget
    Km = keys["mask"]
    body, full = seeded_docs[gadget]
    _, B = _shape(p, G, D)
    assert eng.doc_glwes(B, D) == G
    db, gl = dev_u64(eng, body[:G]), dev_u64(eng, full[:G])
    Lb = _lib.lib()
    for queries, size, entry, ref in (
            (False, Lb.fhe_glwe_docs_bytes, Lb.fhe_glwe_docs_pack_seeded, eng.pack_docs_glwe),
            (True, Lb.fhe_glwe_docs_queries_bytes, Lb.fhe_glwe_docs_queries_pack_seeded, eng.pack_docs_glwe_queries)):
        want = ref(gl, B, D, beta, L).cpu().numpy()
        got = eng.pack_docs_glwe_seeded(db, DOC_ID0, Km, B, D, beta, L, queries=queries).cpu().numpy()
        assert got.dtype == np.uint8 and got.size == want.size
        np.testing.assert_array_equal(got, want, err_msg=f"queries={queries}")
        n = size(C.byref(eng._P), B, D, L)
        assert n == want.size
        buf = torch.full((n + 16,), SENT, dtype=torch.uint8, device=eng.device)
        eng._chk(entry(eng._ctx, db.data_ptr(), C.c_uint64(DOC_ID0), B, D, beta, L, eng._key(Km), buf.data_ptr(), None))
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        np.testing.assert_array_equal(out[:n], want)
        assert (out[n:] == SENT).all()


@pytest.mark.parametrize("gadget,Qn,G,D", [((4, 3), 1, 2, 5), ((7, 7), 3, 17, 16), ((4, 3), 6, 1, 256),
                                           ((7, 7), 6, 2, 1)])
def test_leveled_step_on_seeded_inputs(toy, keys, seeded_docs, gadget, Qn, G, D):
    """linear_ggsws and linear_ggsw on expanded seeded queries and document
    operands made from the bodies equal the full-form calls and the
    restatement (its own expansion, then tests/extprod_ref.py) word for word."""
    eng = toy
    p = eng.params
    beta, L = gadget
    Km, Kn = keys["mask"], keys["noise"]
    body, full = seeded_docs[gadget]
    _, B = _shape(p, G, D)
    rng = np.random.default_rng(7 * beta + Qn)
    ids = QUERY_IDS[:Qn]
    qb = np.stack([u64(eng.encrypt_ggsw_seeded(rng.integers(-2 ** 12, 2 ** 12, 16), beta, L, Km, Kn, i)) for i in ids])
    for i, w in enumerate(EDGE_WORDS):                     # edge words in the bodies of several queries
        qb[i % Qn, (i + 1) % ((p.k + 1) * L), 3 * i:3 * i + 2] = U(w)
    ggsws = eng.expand_ggsws_seeded(dev_u64(eng, qb), ids, beta, L, Km)
    ref_g = np.stack([S.expand_ggsw(qb[q], Km, ids[q], p.N, p.k, L) for q in range(Qn)])
    np.testing.assert_array_equal(u64(ggsws).reshape(ref_g.shape), ref_g)
    db, gl = dev_u64(eng, body[:G]), dev_u64(eng, full[:G])
    csts = [-37, 5, 0, 11, -1, 300][:Qn]
    docs_s = eng.pack_docs_glwe_seeded(db, DOC_ID0, Km, B, D, beta, L, queries=True)
    docs_f = eng.pack_docs_glwe_queries(gl, B, D, beta, L)
    got = u64(eng.linear_ggsws(ggsws, beta, L, docs_s, B, D, csts)).reshape(Qn, B, -1)
    np.testing.assert_array_equal(got, u64(eng.linear_ggsws(ggsws, beta, L, docs_f, B, D, csts)).reshape(Qn, B, -1))
    docs8_s = eng.pack_docs_glwe_seeded(db, DOC_ID0, Km, B, D, beta, L)
    for q in range(Qn):
        want = X.extract_slots(X.external_product(full[:G], ref_g[q], beta), B, D,
                               (csts[q] << (64 - p.msg_bits)) % 2 ** 64)
        np.testing.assert_array_equal(got[q], want, err_msg=f"query {q} against the restatement")
        one = u64(eng.linear_ggsw(ggsws[q], beta, L, docs8_s, B, D, csts[q]))
        np.testing.assert_array_equal(got[q], one, err_msg=f"query {q} against linear_ggsw")


@pytest.fixture(scope="module")
def private16(need_gpu):
    """The 16-dim, n_bits 6 model of tests/test_gpu_private_queries.py (its
    recipe, copied) with a seeded client; the packing key planned for 3 x 64
    results in one GLWE."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.private import PrivateClient
    tfhe_ref.build()
    Xt, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(Xt, y, 6)
    oq = Q.fit_quantized_linear(Xt, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client = PrivateClient(c, count=256, pack_seed=4, enc_seed=12, seeded=True, mask_seed=13)
    return c, client, oq


def test_seeded_search_end_to_end_on_evaluation_only_server(private16):
    """PrivateClient(seeded=True), an evaluation-only PrivateServer, Q = 3 x
    B = 64 at P0 = 21, gadget (7, 6): the replies decrypt to quant_ref's
    accumulators and threshold bits, and they equal, word for word, the
    replies to version-1 payloads holding the same words (the seeded payloads
    expanded on this side by the restatement). The single-query entry too."""
    from fheicp import private as P
    c, client, oq = private16
    assert client.gadget == (7, 6) and c.P0 == 21
    N, k, L = c.scheme.N, c.scheme.k, 6
    s_e = c.cq.s_e
    q0, docs = Q.make_corpus(16, 64, seed=21)
    queries = np.stack([q0, Q.make_corpus(16, 64, seed=31)[0], Q.make_corpus(16, 64, seed=32)[0]])
    ref_acc = np.stack([Q.corpus_accumulate(oq, s_e, 6, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, s_e)) * ref_acc.astype(np.float64)
    ts = [0.5, float(np.median(scores[1])), None]
    want = np.stack([(scores[q] < ts[q]).astype(np.int64) if ts[q] is not None else np.zeros(64, np.int64)
                     for q in range(3)])
    assert 0.25 <= want[1].mean() <= 0.75
    block = client.encrypt_docs(docs, id0=2 ** 64 - 1)
    payloads = client.encrypt_queries(queries, id0=2 ** 64 - 40)       # the id ranges cross the wrap
    # the payload bytes: N words per document GLWE, (k+1) L N per query, beside the headers
    assert 8 * (block.size - P.SEEDED_HEADER_WORDS) == 8192 and 8 * (payloads[0].size - P.SEEDED_HEADER_WORDS) == 147456
    bl = P.unpack_doc_block_seeded(block)
    np.testing.assert_array_equal(client.decrypt_docs(block), c.cq.quant(docs))
    server = P.PrivateServer(client.eval_keys(), c.cq, c.P0, device=0, scheme=c.scheme)
    docs_op, B = server.pack_docs_many(block)
    assert B == 64
    replies = server.search_many(payloads, docs_op, B, ts)
    acc, below = client.decrypt_replies(replies)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref_acc)
    np.testing.assert_array_equal(below.cpu().numpy(), want)
    # the same words as version-1 payloads
    full_block = P.pack_doc_block(S.expand_glwe(bl["body"], bl["mask_key"], bl["id0"], N, k), 64, 16, c.P0, N, k)
    assert 8 * (full_block.size - P.HEADER_WORDS) == 24576
    full_payloads = []
    for pay in payloads:
        pl = P.unpack_ggsw_query_seeded(pay)
        full_payloads.append(P.pack_ggsw_query(S.expand_ggsw(pl["body"], pl["mask_key"], pl["id0"], N, k, L), 16,
                                               c.P0, 7, L, N, k))
    assert 8 * (full_payloads[0].size - P.HEADER_WORDS) == 442368
    fdocs, _ = server.pack_docs_many(full_block)
    assert torch.equal(fdocs, docs_op)
    full_replies = server.search_many(full_payloads, fdocs, B, ts)
    assert len(replies) == len(full_replies) == 1
    np.testing.assert_array_equal(replies[0], full_replies[0])
    # one query through search / pack_docs
    d8, _ = server.pack_docs(block)
    f8, _ = server.pack_docs(full_block)
    assert torch.equal(d8, f8)
    np.testing.assert_array_equal(server.search(payloads[1], d8, B, ts[1]), server.search(full_payloads[1], f8, B, ts[1]))
    # what the host refuses
    with pytest.raises(ValueError, match="query 1: a full-form payload"):
        server.search_many([payloads[0], full_payloads[1]], docs_op, B, None)
    with pytest.raises(ValueError, match="query 1: stream ids"):
        server.search_many([payloads[0], payloads[0]], docs_op, B, None)
    with pytest.raises(ValueError, match="document block: stream ids"):
        server.pack_docs_many(client.encrypt_docs(docs[:5], id0=2 ** 64 - 1))
    server.engine.close()


def test_hub_with_a_seeded_and_a_full_form_tenant(need_gpu):
    """PrivateHub on the 5-feature, 2-bit model of tests/test_gpu_private_hub.py
    (P0 = 8): alice sends seeded blocks and queries, bob full-form ones, in one
    grouped call; each tenant's reply equals its own PrivateServer.search_many
    word for word and decrypts to the clear restatement."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.model import QuantParams
    from fheicp.private import SEEDED_DOCS_MAGIC, DOCS_MAGIC, PrivateClient, PrivateHub
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    cq = CorpusQuant(qp, 2, 0.5)
    oq = Q.QuantizedLinearParams.from_json(qp.to_dict())
    hub, requests, want, clients = PrivateHub(0), {}, {}, {}
    for i, (name, Qn, B, seeded) in enumerate((("alice", 3, 130, True), ("bob", 2, 17, False))):
        rng = np.random.default_rng(77 + i)
        qs = rng.uniform(-1.2, 0.7, (Qn, 5)).astype(np.float32)
        docs = rng.uniform(-1.2, 0.7, (B, 5)).astype(np.float32)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 2, q, docs) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        ts = [None, float(np.median(scores[1])), 0.5][:Qn]
        c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=99 + i, device=0, noise_seed=6 + i)
        client = PrivateClient(c, count=TOY.N, pack_seed=17 + i, enc_seed=12 + i, seeded=seeded, mask_seed=40 + i)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, scheme=c.scheme)
        block = client.encrypt_docs(docs)
        assert int(block[0]) == (SEEDED_DOCS_MAGIC if seeded else DOCS_MAGIC)
        assert hub.load(name, block) == B
        requests[name] = (client.encrypt_queries(qs), ts)
        want[name] = (ref, np.stack([np.zeros(B, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                                     for q, t in enumerate(ts)]))
        clients[name] = client
    got = hub.search_many(requests)
    first = next(iter(hub.tenants.values()))["server"].engine
    assert first.kernel_name("linear_ggsws").startswith("k_extprod_queries_mfma_grp<")   # the hub ran the group form
    assert first.kernel_name("expand_ggsw_seeded") == "k_expand_ggsw_seeded"             # alice's, on her own context
    for name, client in clients.items():
        rec = hub.tenants[name]
        own = rec["server"].search_many(requests[name][0], rec["docs"], rec["B"], requests[name][1])
        assert len(got[name]) == len(own) == 1
        np.testing.assert_array_equal(got[name][0], own[0], err_msg=f"{name}: reply words against its own server")
        acc, below = client.decrypt_replies(got[name])
        np.testing.assert_array_equal(acc.cpu().numpy(), want[name][0], err_msg=name)
        np.testing.assert_array_equal(below.cpu().numpy(), want[name][1], err_msg=name)
    assert 0 < want["alice"][1][1].sum() < 130
    with pytest.raises(ValueError, match="tenant 'alice': query 1: a full-form payload"):
        hub.search_many({"alice": ([requests["alice"][0][0], requests["bob"][0][0]], None)})
    hub.close()


def test_integration_binding_seeded(need_gpu):
    """integration/fhe_gpu.py's seeded calls (numpy and ctypes only) on TOY at
    12 bits: the operands and packed replies of the seeded entries equal those
    of the full-form entries on the expansion, and decrypt to the clear sums."""
    import sys
    from pathlib import Path
    from fheicp import LIB_PATH
    from fheicp.params import extprod_plan, extprod_var
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "integration"))
    from fhe_gpu import GpuCompare
    p = TOY.with_msg_bits(12)
    eng = GpuCompare(p.as_dict(), key_seed=31, lib_path=str(LIB_PATH), enc_seed=1)
    try:
        rng = np.random.default_rng(9)
        Qn, B, D = 3, 70, 5                               # S = 51 per GLWE: two GLWEs
        dq, W = rng.integers(-8, 8, (B, D)), rng.integers(-9, 10, (Qn, D))
        cst, Ts = 11, [-20, 0, 35]
        want = dq @ W.T + cst
        w2 = max(0.5 * (float(np.sum(w * w)) + float(np.abs(w).sum()) ** 2) for w in W)
        beta, L = extprod_plan(p, w2)
        _, _, lb = eng.keygen_pack(count=Qn * B, in_var=extprod_var(p, w2, beta, L) / 2.0 ** 128, seed=32)
        Km, Kn = tfhe_ref.key_from_seed(5), tfhe_ref.key_from_seed(6)
        body, did = eng.encrypt_docs_glwe_seeded(dq, Km, Kn)
        qb, qids = zip(*[eng.encrypt_ggsw_seeded(w, beta, L, Km, Kn) for w in W])
        qb = np.stack(qb)
        assert body.size == 2 * p.N and qb.shape == (Qn, (p.k + 1) * L * p.N)
        docs = eng.pack_docs_glwe_seeded(body, did, Km, B, D, beta, L, queries=True)
        ga, gb = eng.search_ggsws_seeded(qb, qids, Km, beta, L, docs, cst, Ts, lb)
        fdocs = eng.pack_docs_glwe_queries(eng.expand_docs_glwe_seeded(body, did, Km), B, D, beta, L)
        fa, fb = eng.search_ggsws(eng.expand_ggsws_seeded(qb, qids, beta, L, Km), beta, L, fdocs, cst, Ts, lb)
        d8 = eng.pack_docs_glwe_seeded(body, did, Km, B, D, beta, L)
        a1, b1 = eng.search_ggsw_seeded(qb[1], qids[1], Km, beta, L, d8, cst, Ts[1], lb)
        acc = eng.decrypt_packed(ga, Qn * B, 0).reshape(Qn, B) + np.array(Ts)[:, None]
        below = eng.decrypt_packed(gb, Qn * B, 1).reshape(Qn, B)
        acc1 = eng.decrypt_packed(a1, B, 0) + Ts[1]
        for d in (docs, fdocs, d8):
            eng.free_docs(d)
    finally:
        eng.close()
    np.testing.assert_array_equal(ga, fa)
    np.testing.assert_array_equal(gb, fb)
    np.testing.assert_array_equal(acc, want.T)
    np.testing.assert_array_equal(acc1, want.T[1])
    np.testing.assert_array_equal(below, (want.T < np.array(Ts)[:, None]).astype(np.int64))
