"""GPU: key rotation of the stored-ciphertext store through the bridge key
switch.

fhe_bridge_batch is bit-identical to the numpy restatement (tests/bridge_ref.py)
on a key imported from numpy, on TOY (513 columns: the padded column block)
and on sampled columns of the P = 26 parameters; the row map touches the old
documents' rows only; the generated key's rows decrypt to their messages; the
bridge's noise is the model's; and an evaluation-only CorpusServer that was
rekeyed answers, for old and new documents alike, what the clear restatement
(quant_ref.corpus_*) and a freshly encrypted store answer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bridge_ref as BR
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine
from fheicp.params import TOY, bridge_plan, params_for_bits

pytestmark = pytest.mark.gpu

U = np.uint64
CANARY = 0x5EA15EA15EA15EA1
EDGE_ROWS = {0: 0x8080808080808080, 14: 0x7F7F7F7F7F7F7F7F, 16: 0xFFFFFFFFFFFFFFFF, 128: 0,
             255: 0x8080808080808080, 256: 0x7F7F7F7F7F7F7F7F, 299: 0xFFFFFFFFFFFFFFFF}
COUNTS = (1, 15, 16, 17, 129, 300)


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def host_u64(t):
    return t.cpu().numpy().view(U)


def s_big_of(eng) -> np.ndarray:
    s = np.zeros(eng.big, U)
    eng._chk(eng._L.fhe_export_keys(eng._ctx, None, C.c_void_p(s.ctypes.data), None, None))
    return s


def canary_buf(eng, rows):
    return torch.full((rows, eng.W), np.array(CANARY, U).view(np.int64).item(), dtype=torch.int64, device=eng.device)


# ------------------------------------------------------ bit-exact on TOY --
@pytest.fixture(scope="module")
def toy(need_gpu):
    """An evaluation-only TOY context: the bridge needs no key but its own."""
    return Engine(TOY, 0)


@pytest.fixture(scope="module")
def toy_inputs():
    """900 rows of random words with rows forced to the edge words (digits at
    both ends of their range, ties with both coins)."""
    rng = np.random.default_rng(41)
    ct = rng.integers(0, 2 ** 64, (900, TOY.k * TOY.N + 1), dtype=U)
    for r, word in EDGE_ROWS.items():
        ct[r, :] = U(word)
    return ct


@pytest.fixture(scope="module", params=[(4, 3), (7, 6)], ids=["b4l3", "b7l6"])
def toy_bridged(request, toy, toy_inputs):
    """TOY with a numpy-made bridge key of the given gadget imported, and the
    restatement of the first 300 inputs, computed once."""
    beta, lv = request.param
    rng = np.random.default_rng(1000 + beta)
    big = TOY.k * TOY.N
    s_old, s_new = rng.integers(0, 2, big, dtype=U), rng.integers(0, 2, big, dtype=U)
    bk = BR.make_bridge_key(rng, s_old, s_new, beta, lv, TOY.glwe_noise_bits)
    toy.import_bridge_key(beta, lv, bk)
    want = BR.bridge_ref(toy_inputs[:300], bk, beta, lv)
    want.setflags(write=False)
    return beta, lv, bk, want


@pytest.mark.parametrize("count", COUNTS)
def test_bridge_bit_exact_toy(toy, toy_inputs, toy_bridged, count):
    """Counts around a 16-row MFMA group and a 128-row workgroup; 513 columns:
    33 column blocks, the last one padded. Every count here runs the K-split
    GEMM (atomics into zeroed compact rows). A canary row sits after the
    output."""
    beta, lv, bk, want = toy_bridged
    assert toy.W == 513
    buf = canary_buf(toy, count + 1)
    toy.bridge(dev_u64(toy, toy_inputs[:count]), out=buf[:count])
    got = host_u64(buf)
    np.testing.assert_array_equal(got[:count], want[:count])
    assert (got[count] == U(CANARY)).all()
    if count == 17:                                  # in place: every digit is formed before the copy back
        x = dev_u64(toy, toy_inputs[:count])
        toy.bridge(x, out=x)
        np.testing.assert_array_equal(host_u64(x), want[:count])


def test_bridge_unsplit_gemm_bit_exact_toy(need_gpu, toy_inputs):
    """900 inputs: 8 ciphertext blocks x 33 column blocks leave no room for a K
    split, so the GEMM stores instead of adding (the other GEMM path). On a
    context of its own, with uniform words for a key."""
    beta, lv = 4, 3
    toy = Engine(TOY, 0)
    rng = np.random.default_rng(5)
    bk = rng.integers(0, 2 ** 64, (TOY.k * TOY.N, lv, TOY.k * TOY.N + 1), dtype=U)
    toy.import_bridge_key(beta, lv, bk)
    buf = canary_buf(toy, 901)
    toy.profile(True)
    try:
        toy.bridge(dev_u64(toy, toy_inputs), out=buf[:900])
        prof = toy.profile_read("bridge")
    finally:
        toy.profile(False)
    assert prof["launches"] == 1 and prof["items"] == 900 and prof["total_ms"] > 0
    assert toy.kernel_name("bridge") == "k_keyswitch_mfma<8, 1>"
    got = host_u64(buf)
    np.testing.assert_array_equal(got[:900], BR.bridge_ref(toy_inputs, bk, beta, lv))
    assert (got[900] == U(CANARY)).all()
    toy.close()


@pytest.mark.parametrize("Qn,B,B_old", [(1, 5, 5), (3, 7, 2), (2, 20, 17), (4, 16, 0)])
def test_bridge_row_map(toy, toy_bridged, Qn, B, B_old):
    """Rows {q B + b : b < B_old} equal fhe_bridge_batch on the gathered rows;
    every other row and a trailing canary are untouched."""
    rng = np.random.default_rng(Qn * 100 + B)
    ct = rng.integers(0, 2 ** 64, (Qn * B + 1, toy.W), dtype=U)
    ct[Qn * B] = U(CANARY)
    idx = np.array([q * B + b for q in range(Qn) for b in range(B_old)], dtype=np.int64)
    x = dev_u64(toy, ct)
    toy.bridge_rows(x, Qn, B, B_old)
    got = host_u64(x)
    want = ct.copy()
    if B_old:
        want[idx] = host_u64(toy.bridge(dev_u64(toy, ct[idx])))
        assert not np.array_equal(want[idx], ct[idx])
    np.testing.assert_array_equal(got, want)


# ------------------------------------------- real parameters, sampled columns --
def test_bridge_sampled_columns_p26(need_gpu):
    """P = 26 (kN = 2048, 2049 columns, 129 column blocks), the planned gadget,
    16 ciphertexts: sixty-four sampled columns plus the body column against the
    restatement, whose key is those columns of the imported words."""
    p = params_for_bits(26)
    beta, lv = bridge_plan(p, (2.0 ** -33) ** 2)
    assert (beta, lv) == (7, 5)
    eng = Engine(p, 0)
    big = p.k * p.N
    rng = np.random.default_rng(26)
    bk = rng.integers(0, 2 ** 64, (big, lv, big + 1), dtype=U)
    eng.import_bridge_key(beta, lv, bk)
    ct = rng.integers(0, 2 ** 64, (16, big + 1), dtype=U)
    ct[3, :] = U(0x8080808080808080)
    buf = canary_buf(eng, 17)
    eng.bridge(dev_u64(eng, ct), out=buf[:16])
    got = host_u64(buf)
    cols = np.unique(np.concatenate([rng.choice(np.arange(1, big - 1), 62, replace=False), [0, big - 1, big]]))
    assert len(cols) == 65 and cols[-1] == big       # 64 mask columns, both ends among them, and the body
    np.testing.assert_array_equal(got[:16][:, cols], BR.bridge_ref(ct, bk, beta, lv, cols=cols))
    assert (got[16] == U(CANARY)).all()
    eng.close()


# ------------------------------------------------------------- GPU keygen --
@pytest.fixture(scope="module")
def p16_pair(need_gpu):
    """Two key holders on the P = 16 parameters."""
    p = params_for_bits(16)
    A, B = Engine(p, 0), Engine(p, 0)
    A.keygen(501)
    B.keygen(502)
    return p, A, B


def check_keygen(p, eng, s_old, beta, lv):
    big = p.k * p.N
    s_new = s_big_of(eng)
    eng.keygen_bridge_key(s_old, beta, lv, seed=5)
    bk = eng.export_bridge_key()
    assert bk.size == big * lv * (big + 1) == eng.bridge_key_words(beta, lv)
    ph = BR.lwe_phase(bk.reshape(-1, big + 1), s_new).reshape(big, lv)
    with np.errstate(over="ignore"):
        for l in range(lv):
            ph[:, l] -= s_old << U(64 - beta * (l + 1))
    noise = ph.astype(np.int64)
    assert np.abs(noise).max() <= 1 << p.glwe_noise_bits
    assert noise.std() > 0.3 * (1 << p.glwe_noise_bits) and len(np.unique(bk[:64])) == 64
    # export and import round-trip the words, on a context without any other key
    S = Engine(p, 0)
    S.import_bridge_key(beta, lv, bk)
    np.testing.assert_array_equal(S.export_bridge_key(), bk)
    S.close()
    eng.keygen_bridge_key(s_old, beta, lv, seed=5)
    np.testing.assert_array_equal(eng.export_bridge_key(), bk)           # the same seed: the same key
    eng.keygen_bridge_key(s_old, beta, lv, seed=6)
    other = eng.export_bridge_key()
    assert (other != bk).mean() > 0.99                                   # another seed: another key
    eng.keygen_bridge_key(s_old, beta, lv)                               # a 256-bit key from the OS
    assert (eng.export_bridge_key() != bk).mean() > 0.99


def test_bridge_keygen_toy(need_gpu):
    eng = Engine(TOY, 0)
    eng.keygen(77)
    s_old = np.random.default_rng(3).integers(0, 2, eng.big, dtype=U)
    check_keygen(TOY, eng, s_old, 4, 3)
    check_keygen(TOY, eng, s_old, 7, 6)
    eng.close()


def test_bridge_keygen_p16(p16_pair):
    p, A, B = p16_pair
    check_keygen(p, B, s_big_of(A), *bridge_plan(p, 0.0))


def test_bridge_noise_p16(p16_pair):
    """4096 encryptions of random messages under key A, bridged to key B: the
    sigma of (phase under B) - (phase under A) is the model's to within 10%
    (sampling error 1.1%), and every message decrypts under B."""
    p, A, B = p16_pair
    beta, lv = bridge_plan(p, 0.0)
    B.keygen_bridge_key(s_big_of(A), beta, lv, seed=9)
    P = p.msg_bits
    rng = np.random.default_rng(16)
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), 4096)
    msgs[:4] = (-(1 << (P - 1)), (1 << (P - 1)) - 1, 0, -1)
    ct = A.encrypt(msgs, seed=12, id0=3)
    before = A.phase(ct).cpu().numpy().view(U)
    out = B.bridge(ct)
    after = B.phase(out).cpu().numpy().view(U)
    np.testing.assert_array_equal(B.decrypt(out).cpu().numpy(), msgs)
    np.testing.assert_array_equal(BR.decode(after, P), msgs)
    err = (after - before).astype(np.int64)
    sigma = math.sqrt(BR.bridge_var(p, beta, lv))
    print(f"bridge sigma / model at P = 16, gadget ({beta}, {lv}): {err.std() / sigma:.4f}")
    assert 0.9 * sigma <= err.std() <= 1.1 * sigma
    # and the old key holder cannot read the bridged ciphertexts
    assert not np.array_equal(A.decrypt(out).cpu().numpy(), msgs)


# ------------------------------------------------------------ end to end --
def toy_model():
    """A hand-made 5-feature model small enough for TOY: q_w in {-1, 0, 1},
    2-bit document and query values, P0 = 7."""
    from fheicp.corpus import CorpusQuant
    from fheicp.model import QuantParams
    qp = QuantParams(n_bits=2, coef=np.array([1.0, -1.0, 1.0, 0.0, 1.0]), intercept=1.0, s_x=1.0, zp_x=0, s_w=1.0,
                     q_w=np.array([1, -1, 1, 0, 1], dtype=np.int64), q_b=1)
    cq = CorpusQuant(qp, 2, 1.0)
    assert cq.worst_msg_bits() == 7
    return cq, Q.QuantizedLinearParams.from_json(qp.to_dict())


def restate(oq, cq, queries, docs, ts):
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, cq.n_e, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    below = np.stack([(scores[i] < t).astype(np.int64) if t is not None else np.zeros(len(docs), np.int64)
                      for i, t in enumerate(ts)])
    return ref, below


def check_search(server, client, oq, cq, queries, docs, ts):
    replies = server.search_many(queries, ts)
    acc, below = client.decrypt_replies(replies)
    ref, want_below = restate(oq, cq, queries, docs, ts)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(below.cpu().numpy(), want_below)
    return acc.cpu().numpy(), below.cpu().numpy()


@pytest.fixture(scope="module")
def toy_rotation(need_gpu):
    """Three TOY generations of one store: client 0, its rotation client 1 and
    client 2 = client1.rotate(bridge_from=client0); 12 documents under key 0, 5
    under key 1 and 5 under key 2; three queries with thresholds on both sides
    of the scores."""
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient
    cq, oq = toy_model()
    c0 = EncryptedCorpus(cq, TOY).compile(key_seed=5, device=0, noise_seed=6)
    assert c0.P0 == 7
    client0 = CorpusClient(c0, pack_seed=17)
    rng = np.random.default_rng(8)
    docs = rng.integers(-2, 2, (22, 5)).astype(np.float32)
    queries = np.array([[1, -2, 1, 1, -1], [-2, -2, 1, 0, 1], [1, 1, 1, 1, 1]], np.float32)
    old = client0.encrypt_docs(docs[:12])
    client1 = client0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
    new1 = client1.encrypt_docs(docs[12:17])
    client2 = client1.rotate(key_seed=9, pack_seed=21, bridge_seed=22, noise_seed=23, bridge_from=client0)
    new2 = client2.encrypt_docs(docs[17:])
    scores = np.stack([Q.corpus_accumulate(oq, cq.s_e, cq.n_e, q, docs) for q in queries]).astype(np.float64)
    ts = [float(np.median(scores[0])), None, float(np.median(scores[2])) + 0.5]
    assert 0 < (scores[0][:17] < ts[0]).sum() < 17 and 0 < (scores[2][:17] < ts[2]).sum() < 17
    return {"cq": cq, "oq": oq, "c0": c0, "clients": (client0, client1, client2), "docs": docs, "queries": queries,
            "old": old, "new1": new1, "new2": new2, "ts": ts}


def make_server(f, client):
    from fheicp.stored import CorpusServer
    return CorpusServer(client.eval_keys(), f["cq"], f["c0"].P0, f["c0"].mask_key, scheme=f["c0"].scheme)


def test_rotation_end_to_end_toy(toy_rotation):
    f = toy_rotation
    cq, oq, docs, queries, ts = f["cq"], f["oq"], f["docs"], f["queries"], f["ts"]
    client0, client1, _ = f["clients"]
    keys1 = client1.eval_keys()
    assert set(keys1) >= {"bridge_key", "bridge_gadget", "bridge_from", "key_id"}
    assert str(keys1["bridge_from"][0]) == client0.key_id == str(client0.eval_keys()["key_id"][0])
    assert len(client0.key_id) == 16 and client1.key_id != client0.key_id
    assert "bridge_key" not in client0.eval_keys()
    # no two documents share a mask stream
    ids_old, ids_new = f["old"][1], f["new1"][1]
    used = {int(i) + j for i in ids_old for j in range(5)}
    assert not used & {int(i) + j for i in ids_new for j in range(5)}
    server = make_server(f, client0)                     # evaluation keys only
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        server.engine.decrypt(server.engine.empty_big(1))
    assert server.load(*f["old"]) == 12
    check_search(server, client0, oq, cq, queries, docs[:12], ts)
    server.rekey(keys1)
    assert server.b_old == 12
    # B_old = B: every document old-generation, and Q = 1
    check_search(server, client1, oq, cq, queries, docs[:12], ts)
    check_search(server, client1, oq, cq, queries[:1], docs[:12], ts[:1])
    one = server.search(queries[0], ts[0])
    acc1, _ = client1.decrypt_replies(one)
    np.testing.assert_array_equal(acc1.cpu().numpy()[0], Q.corpus_accumulate(oq, cq.s_e, cq.n_e, queries[0], docs[:12]))
    # mixed: 12 old + 5 new, Q = 3, mixed thresholds
    assert server.append(*f["new1"]) == 17 and server.b_old == 12
    acc, below = check_search(server, client1, oq, cq, queries, docs[:17], ts)
    assert 0 < below[0].sum() < 17 and below[1].sum() == 0 and 0 < below[2].sum() < 17
    # a second server with all 17 documents freshly encrypted under key 1: the same values
    fresh = make_server(f, client1)
    fresh.load(*client1.encrypt_docs(docs[:17]))
    assert fresh.b_old == 0
    acc2, below2 = check_search(fresh, client1, oq, cq, queries, docs[:17], ts)
    np.testing.assert_array_equal(acc, acc2)
    np.testing.assert_array_equal(below, below2)
    # B_old = 0: the bridged entry is the unbridged entry word for word
    eng = fresh.engine
    Wr, cst, Ts, P = fresh._plan.plan_many(queries, ts)
    eng.set_msg_bits(P)
    Wd = eng.to_dev(Wr)
    ga, gb = eng.search_seeded_queries(fresh.body, fresh.ids, fresh.mask_key, Wd, cst, Ts, fresh.bit_levels)
    ga2, gb2 = torch.zeros_like(ga), torch.zeros_like(gb)
    hT = (C.c_int64 * 3)(*Ts)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert eng._L.fhe_search_seeded_queries_bridged_batch(
        eng._ctx, p(fresh.body), p(fresh.ids), 17, 5, eng._key(fresh.mask_key), 3, p(Wd), cst, hT, fresh.bit_levels, 0,
        p(ga2), p(gb2), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)
    # the old key holder cannot open the new replies
    a0, _ = client0.decrypt_replies(server.search_many(queries, ts))
    assert not np.array_equal(a0.cpu().numpy(), acc)


def test_second_rotation_bridges_from_generation_0(toy_rotation):
    """Generation 0 straight to generation 2 (rotate(bridge_from=first
    client)) with generation-0 documents resident through both rekeys."""
    f = toy_rotation
    cq, oq, docs, queries, ts = f["cq"], f["oq"], f["docs"], f["queries"], f["ts"]
    client0, client1, client2 = f["clients"]
    keys2 = client2.eval_keys()
    assert str(keys2["bridge_from"][0]) == client0.key_id
    # ids continue after both earlier generations
    used = {int(i) + j for part in (f["old"], f["new1"]) for i in part[1] for j in range(5)}
    assert not used & {int(i) + j for i in f["new2"][1] for j in range(5)}
    server = make_server(f, client0)
    server.load(*f["old"])
    server.rekey(client1.eval_keys())
    server.rekey(keys2)
    assert (server.b_old, server.old_key_id, server.key_id) == (12, client0.key_id, client2.key_id)
    assert server.append(*f["new2"]) == 17
    d = np.concatenate([docs[:12], docs[17:]])
    acc, below = check_search(server, client2, oq, cq, queries, d, ts)
    fresh = make_server(f, client2)
    fresh.load(*client2.encrypt_docs(d))
    acc2, below2 = check_search(fresh, client2, oq, cq, queries, d, ts)
    np.testing.assert_array_equal(acc, acc2)
    np.testing.assert_array_equal(below, below2)
    # a bridge from generation 1 does not fit generation-0 documents
    s2 = make_server(f, client0)
    s2.load(*f["old"])
    with pytest.raises(ValueError, match="bridge key comes from"):
        s2.rekey(client1.rotate(key_seed=11, pack_seed=1, bridge_seed=2, noise_seed=3).eval_keys())


def test_bridge_device_refusals(toy_rotation):
    f = toy_rotation
    client0, client1, _ = f["clients"]
    server = make_server(f, client0)                     # evaluation keys of generation 0: no bridge key
    server.load(*f["old"])
    eng = server.engine
    Wr, cst, Ts, P = server._plan.plan_many(f["queries"], f["ts"])
    eng.set_msg_bits(P)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no bridge key"):
        eng.search_seeded_queries(server.body, server.ids, server.mask_key, eng.to_dev(Wr), cst, Ts, server.bit_levels,
                                  b_old=3)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no bridge key"):
        eng.bridge(eng.empty_big(4))
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no bridge key"):
        eng.export_bridge_key()
    with pytest.raises(_lib.FheError, match="FHE_E_ARG"):
        eng.search_seeded_queries(server.body, server.ids, server.mask_key, eng.to_dev(Wr), cst, Ts, server.bit_levels,
                                  b_old=13)
    # key generation needs the new secret: not on an evaluation-only context
    s_old = np.zeros(eng.big, U)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no secret key"):
        eng.keygen_bridge_key(s_old, 4, 3, seed=1)
    s_old[5] = 2
    with pytest.raises(_lib.FheError, match="FHE_E_ARG"):
        eng.keygen_bridge_key(s_old, 4, 3, seed=1)
    # rotate() needs a client whose secret is still held
    from fheicp.stored import CorpusClient
    gone = CorpusClient.__new__(CorpusClient)
    gone.__dict__.update(client0.__dict__)
    gone.corpus = type(client0.corpus)(f["cq"], TOY)      # never compiled: no secret
    with pytest.raises(RuntimeError, match="not compiled"):
        client1.rotate(key_seed=1, bridge_from=gone)


def test_rotation_end_to_end_real_parameters(need_gpu):
    """The 16-dim n_bits = 6 corpus model (P0 = 21): 24 documents under the
    old key, 16 under the new one, Q = 2; the decrypted values equal the
    restatement."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.stored import CorpusClient, CorpusServer
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    assert c.P0 == 21
    client0 = CorpusClient(c, pack_seed=17)
    q21, docs = Q.make_corpus(16, 40, seed=21)
    queries = np.stack([q21, Q.make_corpus(16, 40, seed=31)[0]])
    server = CorpusServer(client0.eval_keys(), cq, c.P0, c.mask_key)
    server.load(*client0.encrypt_docs(docs[:24]))
    client1 = client0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
    assert client1.bridge_gadget == (7, 5) and client1.margin >= 9.2
    server.rekey(client1.eval_keys())
    server.append(*client1.encrypt_docs(docs[24:]))
    assert (server.b_old, int(server.body.shape[0])) == (24, 40)
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * np.stack(
        [Q.corpus_accumulate(oq, cq.s_e, 6, q, docs) for q in queries]).astype(np.float64)
    ts = [float(np.median(scores[0])), float(np.median(scores[1]))]
    _, below = check_search(server, client1, oq, cq, queries, docs, ts)
    assert below[0].sum() == 20 and below[1].sum() == 20
    assert 0 < below[0][:24].sum() < 24 and 0 < below[0][24:].sum() < 16
