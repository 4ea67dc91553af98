"""GPU: seeded evaluation keys. The seeded keygen against
the one-key keygen under the same streams (the anchor), export / import of
bodies against the numpy restatement (tests/seeded_keys_ref.py) and against
the generating context's full form, the three servers and a hub built from a
seeded dict against servers built from the full form of the same keys, and
what the library and the Python side refuse.

Two small parameter sets: TOY (n = 64, N = 256), and n = 61 with one multi-bit
gadget: an odd pair count, a partly used last ChaCha block and 62-word rows
that are 8-byte aligned and no more. The library admits the multi-bit blind
rotation at N = 1024 only, so the second set is TOY at N = 1024."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import seeded_keys_ref as S
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine
from fheicp.params import TOY

pytestmark = pytest.mark.gpu
U = np.uint64
TOY_MB = replace(TOY, n=61, N=1024, pbs_base_log=12, pbs_level=3, pbs_fast_base_log=8, pbs_fast_level=2,
                 pbs_fast_group=2)
SETS = {"n64": TOY, "n61_multibit": TOY_MB}
SEED = 4321
K = Engine.key_from_seed


def gadget_args(prm, g):
    """(messages of s_small, level, base_log) of bootstrapping key g (0: the main one)."""
    if g == 0:
        return (lambda s: np.asarray(s)), prm.pbs_level, prm.pbs_base_log
    assert g == 1
    return (S.mb_messages if prm.pbs_fast_group == 2 else (lambda s: np.asarray(s))), prm.pbs_fast_level, \
        prm.pbs_fast_base_log


def sample_rows(rows):
    return sorted({0, 1, rows // 2, rows - 2, rows - 1})


@pytest.fixture(scope="module", params=list(SETS), ids=list(SETS))
def pair(request, need_gpu):
    """One engine with the one-key keygen of SEED, one with the seeded keygen
    under mask key = noise key = that seed's key; packing keys at (4, 3) and a
    bridge key at (4, 3) from a fixed old big key on both."""
    prm = SETS[request.param]
    A, B = Engine(prm, 0), Engine(prm, 0)
    A.keygen(seed=SEED)
    B.keygen(seed=SEED, mask_key=K(SEED))
    s_old = np.random.default_rng(5).integers(0, 2, prm.k * prm.N).astype(U)
    yield prm, A, B, s_old
    A.close()
    B.close()


def test_anchor_seeded_keygen_against_one_key_keygen(pair):
    """mask key = noise key = K: ksk, packing and bridge keys are the one-key
    keygen's word for word; every bootstrapping key is the one-key keygen's
    with the messages of its rows c < k moved from the mask to the body
    (seeded_keys_ref.messages_to_body: same streams, noise and phases). The
    seeded export's bodies are the body columns of the full form."""
    prm, A, B, s_old = pair
    N, k, n = prm.N, prm.k, prm.n
    sec = A.export_keys()
    np.testing.assert_array_equal(B.export_key("s_small"), sec["s_small"])
    np.testing.assert_array_equal(B.export_key("s_big"), sec["s_big"])
    fa, fb = A.export_eval_keys(), B.export_eval_keys()
    np.testing.assert_array_equal(fb["ksk"], fa["ksk"])
    for g, name in ((0, "bsk"), (1, "gadget_bsk1")):
        if name not in fa:
            assert prm is TOY and g == 1
            continue
        msgs, L, beta = gadget_args(prm, g)
        want = S.messages_to_body(fa[name], msgs(sec["s_small"]), sec["s_big"], N, k, L, beta)
        assert not np.array_equal(want, fa[name])
        np.testing.assert_array_equal(fb[name], want, err_msg=name)
    sd = B.export_eval_keys(seeded=True)
    assert set(sd) == {"eval_mask_key", "bsk_body", "ksk_body"} | ({"gadget_bsk1_body"} if prm is TOY_MB else set())
    np.testing.assert_array_equal(sd["eval_mask_key"], K(SEED))
    np.testing.assert_array_equal(sd["bsk_body"], S.glwe_row_bodies(fb["bsk"], N, k).reshape(-1))
    np.testing.assert_array_equal(sd["ksk_body"], S.lwe_row_bodies(fa["ksk"], n + 1))
    if prm is TOY_MB:
        np.testing.assert_array_equal(sd["gadget_bsk1_body"], S.glwe_row_bodies(fb["gadget_bsk1"], N, k).reshape(-1))
    # the one-key keygen has no mask key to export
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*seeded"):
        A.export_eval_keys(seeded=True)
    # packing keys at two gadgets, each under its own mask key, and the bridge key
    for i, gad in enumerate(((4, 3), (7, 7))):
        A.keygen_pack(*gad, seed=100 + i)
        B.keygen_pack(*gad, seed=100 + i, mask_key=K(100 + i))
        full = A.export_pack_key()
        np.testing.assert_array_equal(B.export_pack_key(), full)
        mk, body = B.export_pack_key_seeded()
        np.testing.assert_array_equal(mk, K(100 + i))
        np.testing.assert_array_equal(body, S.glwe_row_bodies(full, N, k).reshape(-1))
        with pytest.raises(_lib.FheError, match="FHE_E_STATE.*seeded"):
            A.export_pack_key_seeded()
    A.keygen_bridge_key(s_old, 4, 3, seed=200)
    B.keygen_bridge_key(s_old, 4, 3, seed=200, mask_key=K(200))
    full = A.export_bridge_key()
    np.testing.assert_array_equal(B.export_bridge_key(), full)
    mk, body = B.export_bridge_key_seeded()
    np.testing.assert_array_equal(mk, K(200))
    np.testing.assert_array_equal(body, S.lwe_row_bodies(full, k * N + 1))
    # refusal: a mask key this context's seeded keygens already used
    for used in (SEED, 100, 101, 200):
        with pytest.raises(_lib.FheError, match="FHE_E_ARG.*mask key reuse"):
            B.keygen_pack(4, 3, seed=300, mask_key=K(used))
        with pytest.raises(_lib.FheError, match="FHE_E_ARG.*mask key reuse"):
            B.keygen_bridge_key(s_old, 4, 3, seed=300, mask_key=K(used))
    np.testing.assert_array_equal(B.export_pack_key_seeded()[0], K(101))          # the refused calls changed nothing


@pytest.fixture(scope="module", params=list(SETS), ids=list(SETS))
def shipped(request, need_gpu):
    """A key holder with distinct mask and noise keys (main set, packing key
    (4, 3), bridge key (4, 3)), its seeded dict, and an evaluation-only context
    that imported the dict."""
    prm = SETS[request.param]
    Cn, E = Engine(prm, 0), Engine(prm, 0)
    s_old = np.random.default_rng(6).integers(0, 2, prm.k * prm.N).astype(U)
    Cn.keygen(seed=77, mask_key=K(1001))
    Cn.keygen_pack(4, 3, seed=78, mask_key=K(1002))
    Cn.keygen_bridge_key(s_old, 4, 3, seed=79, mask_key=K(1003))
    d = Cn.export_eval_keys(seeded=True)
    E.keygen(seed=1)                                 # secrets in place: the import must remove them
    E.import_eval_keys(d)
    yield prm, Cn, E, d, s_old
    Cn.close()
    E.close()


def test_import_expands_to_the_generating_contexts_full_form(shipped):
    prm, Cn, E, d, _ = shipped
    N, k, n = prm.N, prm.k, prm.n
    full_c, full_e = Cn.export_eval_keys(), E.export_eval_keys()
    assert set(full_c) == set(full_e) >= {"bsk", "ksk", "pack_key", "pack_gadget", "bridge_key", "bridge_gadget"}
    for name in full_c:
        np.testing.assert_array_equal(full_e[name], full_c[name], err_msg=name)
    assert tuple(full_e["pack_gadget"]) == (4, 3) and tuple(full_e["bridge_gadget"]) == (4, 3)
    # sizes: the ABI's body words, a third of the GLWE-row keys and one word per LWE row
    assert d["bsk_body"].size * (k + 1) == full_c["bsk"].size and d["ksk_body"].size * (n + 1) == full_c["ksk"].size
    assert d["pack_key_body"].size * (k + 1) == full_c["pack_key"].size
    assert d["bridge_key_body"].size * (k * N + 1) == full_c["bridge_key"].size
    # the numpy restatement: the main set word for word; of the packing and
    # bridge keys, whose rows number thousands, rows at both ends and the middle
    mk = d["eval_mask_key"]
    np.testing.assert_array_equal(mk, K(1001))
    np.testing.assert_array_equal(S.expand_lwe_rows(d["ksk_body"], mk, S.TAG_KSK_MASK, n + 1), full_e["ksk"])
    np.testing.assert_array_equal(S.expand_glwe_rows(d["bsk_body"], mk, S.TAG_BSK_MASK, N, k), full_e["bsk"])
    if prm is TOY_MB:
        np.testing.assert_array_equal(S.expand_glwe_rows(d["gadget_bsk1_body"], mk, S.TAG_MB_MASK[1], N, k),
                                      full_e["gadget_bsk1"])
    n1 = (k + 1) * N
    pb, pk = d["pack_key_body"].reshape(-1, N), full_e["pack_key"].reshape(-1, n1)
    for r in sample_rows(len(pb)):
        np.testing.assert_array_equal(S.glwe_row(pb[r], d["pack_mask_key"], S.TAG_PACK_MASK, r, N, k), pk[r], err_msg=r)
    bb, bk = d["bridge_key_body"], full_e["bridge_key"].reshape(-1, k * N + 1)
    for r in sample_rows(len(bb)):
        np.testing.assert_array_equal(S.lwe_row(bb[r], d["bridge_mask_key"], S.TAG_BRIDGE_MASK, r, k * N + 1), bk[r],
                                      err_msg=r)
    # the importing context can ship the keys seeded again: it kept the mask keys
    again = E.export_eval_keys(seeded=True)
    assert set(again) == set(d)
    for name in d:
        np.testing.assert_array_equal(again[name], d[name], err_msg=name)


def test_rows_decrypt_under_the_exported_secrets(shipped):
    """Every ksk and bridge row's phase is its message plus a noise within
    TUniform's bound (2^lwe_noise_bits, 2^glwe_noise_bits), in numpy."""
    prm, Cn, E, _, s_old = shipped
    N, k, n = prm.N, prm.k, prm.n
    sec = Cn.export_keys()
    full = E.export_eval_keys()
    ph = S.lwe_row_phases(full["ksk"], n + 1, sec["s_small"]).reshape(k * N, prm.ks_level)
    msg = sec["s_big"][:, None] << (U(64) - U(prm.ks_base_log) * np.arange(1, prm.ks_level + 1, dtype=U))[None, :]
    assert np.abs((ph - msg).astype(np.int64)).max() <= 2 ** prm.lwe_noise_bits
    ph = S.lwe_row_phases(full["bridge_key"], k * N + 1, sec["s_big"]).reshape(k * N, 3)
    msg = s_old[:, None] << (U(64) - U(4) * np.arange(1, 4, dtype=U))[None, :]
    assert np.abs((ph - msg).astype(np.int64)).max() <= 2 ** prm.glwe_noise_bits


def test_importing_context_holds_no_secret(shipped):
    _, _, E, _, s_old = shipped
    for call in (lambda: E.decrypt(E.empty_big(1)), lambda: E.export_keys(), lambda: E.keygen_pack(4, 3, seed=3),
                 lambda: E.keygen_pack(4, 3, seed=3, mask_key=K(9)),
                 lambda: E.keygen_bridge_key(s_old, 4, 3, seed=3, mask_key=K(9))):
        with pytest.raises(_lib.FheError, match="FHE_E_STATE: no secret key: this context holds evaluation keys only"):
            call()


def test_refusals(need_gpu):
    """Seeded export after fhe_import_keys (the fast gadget's key was
    re-encrypted under a private key; bsk and ksk came without a mask key), a
    body of the wrong size, and a dict of both forms."""
    prm = replace(TOY, pbs_base_log=12, pbs_level=3, pbs_fast_base_log=8, pbs_fast_level=2)
    A, X = Engine(prm, 0), Engine(prm, 0)
    try:
        A.keygen(seed=8, mask_key=K(80))
        d = A.export_eval_keys(seeded=True)
        X.import_keys(A.export_keys())
        with pytest.raises(_lib.FheError, match="FHE_E_STATE.*seeded"):
            X.export_eval_keys(seeded=True)
        # the library's own fast-gadget refusal: a seeded set whose gadget keys were replaced
        X.import_eval_keys(d)
        X.export_eval_keys(seeded=True)
        for name in ("bsk_body", "ksk_body", "gadget_bsk1_body"):
            with pytest.raises(ValueError, match="^" + name + ":"):
                X.import_eval_keys(dict(d, **{name: d[name][:-1]}))
        with pytest.raises(ValueError, match="mix the seeded and the full form"):
            X.import_eval_keys(dict(d, bsk=A.export_key("bsk")))
        A.keygen_pack(4, 3, seed=9, mask_key=K(81))
        d = A.export_eval_keys(seeded=True)
        with pytest.raises(ValueError, match="^pack_key_body:"):
            X.import_eval_keys(dict(d, pack_gadget=np.array([4, 4])))
        buf = np.zeros(4, U)
        assert X._L.fhe_import_pack_key_seeded(X._ctx, 4, 3, None, C.c_void_p(buf.ctypes.data)) == -1
        assert b"seeded" in X._L.fhe_last_error(X._ctx)
    finally:
        A.close()
        X.close()


# ------------------------------------------------------------- end to end --
def toy8_model():
    """The 5-feature, 2-bit model of tests/test_gpu_multi_query.py (P0 = 8 = TOY's width)."""
    from fheicp.corpus import CorpusQuant
    from fheicp.model import QuantParams
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    return CorpusQuant(qp, 2, 0.5), Q.QuantizedLinearParams.from_json(qp.to_dict())


def toy8_inputs(seed, Qn, B):
    cq, oq = toy8_model()
    rng = np.random.default_rng(seed)
    qs = rng.uniform(-1.2, 0.7, (Qn, 5)).astype(np.float32)
    docs = rng.uniform(-1.2, 0.7, (B, 5)).astype(np.float32)
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 2, q, docs) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    ts = [None, float(np.median(scores[1])), 0.5][:Qn]
    below = np.stack([np.zeros(B, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                      for q, t in enumerate(ts)])
    return qs, docs, ts, ref, below


def check_seeded_dict(d, full):
    assert "bsk_body" in d and "pack_key_body" in d and not {"bsk", "ksk", "pack_key"} & set(d)
    assert "bsk" in full and "pack_key" in full and "bsk_body" not in full
    nbytes = lambda x: sum(np.asarray(v).nbytes for v in x.values())   # noqa: E731
    assert 3 * nbytes(d) < nbytes(full)


def test_query_server_from_a_seeded_dict(need_gpu):
    from fheicp.corpus import EncryptedCorpus
    from fheicp.query import QueryClient, QueryServer
    cq, _ = toy8_model()
    qs, docs, ts, ref, below = toy8_inputs(77, 3, 130)
    c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=5, device=0, noise_seed=6, seeded_keys=True,
                                                key_mask_seed=500)
    client = QueryClient(c, count=TOY.N, pack_seed=17)
    d, full = client.eval_keys(), client.eval_keys(seeded=False)
    check_seeded_dict(d, full)
    np.testing.assert_array_equal(d["eval_mask_key"], K(500))
    np.testing.assert_array_equal(d["pack_mask_key"], K(501))
    payloads = client.encrypt_queries(qs)
    replies = []
    for keys in (d, full):
        server = QueryServer(keys, cq, c.P0, scheme=c.scheme)
        replies.append(server.search_many(payloads, server.pack_docs(docs), 130, ts))
        with pytest.raises(_lib.FheError, match="FHE_E_STATE.*secret"):
            server.engine.decrypt(server.engine.empty_big(1))
        server.engine.close()
    assert len(replies[0]) == len(replies[1]) == 1
    np.testing.assert_array_equal(replies[0][0], replies[1][0])
    acc, bl = client.decrypt_replies(replies[0])
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(bl.cpu().numpy(), below)
    assert 0 < below[1].sum() < 130


def private_tenant(i, seeded_keys, Qn, B):
    from fheicp.corpus import EncryptedCorpus
    from fheicp.private import PrivateClient
    cq, _ = toy8_model()
    qs, docs, ts, ref, below = toy8_inputs(77 + i, Qn, B)
    c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=99 + i, device=0, noise_seed=6 + i, seeded_keys=seeded_keys,
                                                key_mask_seed=600 + 10 * i)
    client = PrivateClient(c, count=TOY.N, pack_seed=17 + i, enc_seed=12 + i, seeded=False, mask_seed=40 + i)
    return c, cq, client, client.encrypt_docs(docs), client.encrypt_queries(qs), ts, ref, below


def test_private_server_from_a_seeded_dict(need_gpu):
    from fheicp.private import PrivateServer
    c, cq, client, block, payloads, ts, ref, below = private_tenant(0, True, 3, 130)
    d, full = client.eval_keys(), client.eval_keys(seeded=False)
    check_seeded_dict(d, full)
    replies = []
    for keys in (d, full):
        server = PrivateServer(keys, cq, c.P0, device=0, scheme=c.scheme)
        docs_op, B = server.pack_docs_many(block)
        replies.append(server.search_many(payloads, docs_op, B, ts))
        server.engine.close()
    assert len(replies[0]) == len(replies[1])
    for a, b in zip(*replies):
        np.testing.assert_array_equal(a, b)
    acc, bl = client.decrypt_replies(replies[0])
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(bl.cpu().numpy(), below)


def test_hub_with_a_seeded_and_a_full_form_tenant(need_gpu):
    from fheicp.private import PrivateHub
    hub, requests, want, clients = PrivateHub(0), {}, {}, {}
    for i, (name, Qn, B, seeded) in enumerate((("alice", 3, 130, True), ("bob", 2, 17, False))):
        c, cq, client, block, payloads, ts, ref, below = private_tenant(i, seeded, Qn, B)
        keys = client.eval_keys()
        assert ("bsk_body" in keys) == seeded and ("bsk" in keys) != seeded
        hub.add_tenant(name, keys, cq, c.P0, scheme=c.scheme)
        assert hub.load(name, block) == B
        requests[name], want[name], clients[name] = (payloads, ts), (ref, below), client
    got = hub.search_many(requests)
    for name, client in clients.items():
        rec = hub.tenants[name]
        own = rec["server"].search_many(requests[name][0], rec["docs"], rec["B"], requests[name][1])
        assert len(got[name]) == len(own) == 1
        np.testing.assert_array_equal(got[name][0], own[0], err_msg=name)
        acc, bl = client.decrypt_replies(got[name])
        np.testing.assert_array_equal(acc.cpu().numpy(), want[name][0], err_msg=name)
        np.testing.assert_array_equal(bl.cpu().numpy(), want[name][1], err_msg=name)
    hub.close()


def test_corpus_server_rotate_and_rekey_with_seeded_keys(need_gpu):
    """The TOY store of tests/test_gpu_bridge.py with seeded keys: generation 0,
    its rotation (seeded too, with a seeded bridge key), 12 old-generation rows
    resident through the rekey and 5 new ones appended; a server fed seeded
    dicts against one fed the full form of the same keys."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.model import QuantParams
    from fheicp.stored import CorpusClient, CorpusServer
    qp = QuantParams(n_bits=2, coef=np.array([1.0, -1.0, 1.0, 0.0, 1.0]), intercept=1.0, s_x=1.0, zp_x=0, s_w=1.0,
                     q_w=np.array([1, -1, 1, 0, 1], dtype=np.int64), q_b=1)
    cq = CorpusQuant(qp, 2, 1.0)
    oq = Q.QuantizedLinearParams.from_json(qp.to_dict())
    c0 = EncryptedCorpus(cq, TOY).compile(key_seed=5, device=0, noise_seed=6, seeded_keys=True, key_mask_seed=700)
    client0 = CorpusClient(c0, pack_seed=17)
    docs = np.random.default_rng(8).integers(-2, 2, (17, 5)).astype(np.float32)
    queries = np.array([[1, -2, 1, 1, -1], [-2, -2, 1, 0, 1], [1, 1, 1, 1, 1]], np.float32)
    old = client0.encrypt_docs(docs[:12])
    client1 = client0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
    new1 = client1.encrypt_docs(docs[12:])
    assert client1.corpus.seeded_keys and client1.corpus.key_mask_seed == 716
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, cq.n_e, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    ts = [float(np.median(scores[0])), None, float(np.median(scores[2])) + 0.5]
    below = np.stack([(scores[i] < t).astype(np.int64) if t is not None else np.zeros(17, np.int64)
                      for i, t in enumerate(ts)])
    k0, k1 = client0.eval_keys(), client1.eval_keys()
    f0, f1 = client0.eval_keys(seeded=False), client1.eval_keys(seeded=False)
    assert "bridge_key_body" in k1 and "bridge_mask_key" in k1 and "bridge_key" not in k1 and "bridge_key" in f1
    assert "bridge_key_body" not in k0
    np.testing.assert_array_equal(k1["bridge_mask_key"], K(718))
    np.testing.assert_array_equal(k1["eval_mask_key"], K(716))
    # key_id: the fingerprint of the full-form ksk in both forms
    assert str(k0["key_id"][0]) == str(f0["key_id"][0]) == client0.key_id
    assert str(k1["bridge_from"][0]) == client0.key_id and str(k1["key_id"][0]) == client1.key_id != client0.key_id
    servers = [CorpusServer(keys, cq, c0.P0, c0.mask_key, scheme=c0.scheme)
               for keys in (k0, f0, {k: v for k, v in k0.items() if k != "key_id"})]
    assert [s.key_id for s in servers] == [client0.key_id] * 3           # the last one from the expanded key
    servers.pop().engine.close()
    for s in servers:
        assert s.load(*old) == 12
    r0 = [s.search_many(queries, ts) for s in servers]
    for s, keys in zip(servers, (k1, f1)):
        s.rekey(keys)
        assert s.b_old == 12 and s.key_id == client1.key_id and s.old_key_id == client0.key_id
        assert s.append(*new1) == 17
    r1 = [s.search_many(queries, ts) for s in servers]
    for got in (r0, r1):
        assert len(got[0]) == len(got[1])
        for a, b in zip(*got):
            np.testing.assert_array_equal(a, b)
    acc, bl = client0.decrypt_replies(r0[0])
    np.testing.assert_array_equal(acc.cpu().numpy(), ref[:, :12])
    np.testing.assert_array_equal(bl.cpu().numpy(), below[:, :12])
    acc, bl = client1.decrypt_replies(r1[0])
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(bl.cpu().numpy(), below)
    assert 0 < below[0].sum() < 17
    for s in servers:
        s.engine.close()


def test_integration_binding_seeded_import(need_gpu):
    """integration/fhe_gpu.py (numpy and ctypes only): import_eval_keys_seeded
    leaves the full form of the key holder's keys and no secret."""
    import sys
    from pathlib import Path
    from fheicp import LIB_PATH
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "integration"))
    from fhe_gpu import GpuCompare
    A = Engine(TOY, 0)
    A.keygen(seed=21, mask_key=K(22))
    A.keygen_pack(4, 3, seed=23, mask_key=K(24))
    d, full = A.export_eval_keys(seeded=True), A.export_eval_keys()
    A.close()
    g = GpuCompare(TOY.as_dict(), key_seed=31, lib_path=str(LIB_PATH), enc_seed=1)
    try:
        g.import_eval_keys_seeded(d)
        bsk, ksk, pk = (np.zeros_like(full[n]) for n in ("bsk", "ksk", "pack_key"))
        vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731  (the binding declares no fhe_export_keys)
        assert g.L.fhe_export_keys(g.ctx, None, None, vp(bsk), vp(ksk)) == 0
        assert g.L.fhe_export_pack_key(g.ctx, vp(pk)) == 0
        s = np.zeros(TOY.n, U)
        assert g.L.fhe_export_keys(g.ctx, vp(s), None, None, None) == -3               # FHE_E_STATE: no secret
        with pytest.raises(ValueError, match="^ksk_body:"):
            g.import_eval_keys_seeded(dict(d, ksk_body=d["ksk_body"][1:]))
    finally:
        g.close()
    for got, name in ((bsk, "bsk"), (ksk, "ksk"), (pk, "pack_key")):
        np.testing.assert_array_equal(got, full[name], err_msg=name)
