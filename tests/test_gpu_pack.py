"""GPU: the two-party private query through libfheicp.

The packing key switch is bit-identical to the numpy restatement
(tests/pack_ref.py, pinned to the oracle by tests/test_pack_cpu.py) on the
exported key; its key rows, its decryption and its noise follow the
definition and the model; an evaluation-only context computes what the key
holder's context computes and refuses everything that needs the secret; and a
QueryServer built from an .npz of evaluation keys answers a search whose
decrypted reply equals the single-party compare and the clear restatement."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pack_ref as R
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine
from fheicp.params import TOY, pack_plan, params_for_bits

pytestmark = pytest.mark.gpu

U = np.uint64
EDGE_ROWS = {0: 0x8080808080808080, 14: 0x7F7F7F7F7F7F7F7F, 16: 0xFFFFFFFFFFFFFFFF, 128: 0,
             255: 0x8080808080808080, 256: 0x7F7F7F7F7F7F7F7F, 299: 0xFFFFFFFFFFFFFFFF}
COUNTS = (1, 15, 16, 17, 127, 129, 255, 256, 257, 300)


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def host_u64(t):
    return t.cpu().numpy().view(U)


def s_big_of(eng) -> np.ndarray:
    s = np.zeros(eng.big, U)
    eng._chk(eng._L.fhe_export_keys(eng._ctx, None, C.c_void_p(s.ctypes.data), None, None))
    return s


def pack_key_of(eng) -> np.ndarray:
    b, lv = eng.pack_gadget
    p = eng.params
    return eng.export_pack_key().reshape(p.k * p.N, lv, p.k + 1, p.N)


@pytest.fixture(scope="module")
def toy(need_gpu):
    eng = Engine(TOY, 0)
    eng.keygen(99)
    return eng


@pytest.fixture(scope="module")
def toy_inputs(toy):
    """300 TOY ciphertexts, values over the whole msg_bits range, with rows
    forced to the edge words; (messages of the clean rows, host words)."""
    P = TOY.msg_bits
    rng = np.random.default_rng(41)
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), 300)
    msgs[1:5] = (-(1 << (P - 1)), (1 << (P - 1)) - 1, 0, -1)
    ct = host_u64(toy.encrypt(msgs, seed=12, id0=3)).reshape(300, toy.W).copy()
    for r, word in EDGE_ROWS.items():
        ct[r, :] = U(word)
    return msgs, ct


@pytest.fixture(scope="module", params=[(4, 3), (7, 6)], ids=["b4l3", "b7l6"])
def toy_packed(request, toy, toy_inputs):
    """TOY with a packing key of the given gadget, the exported key and the
    restatement's GEMM rows of the 300 inputs for every level count used."""
    beta, lv = request.param
    toy.keygen_pack(beta, lv, seed=1000 + beta)
    pk = pack_key_of(toy)
    rows = {L: R.gemm_rows(toy_inputs[1], pk, beta, L) for L in sorted({lv, 1, lv - 1})}
    return beta, lv, pk, rows


@pytest.mark.parametrize("count", COUNTS)
def test_pack_bit_exact_toy(toy, toy_inputs, toy_packed, count):
    """Counts around a 16-row MFMA group, a 128-row workgroup, a full GLWE
    (the wrap of X^j with its sign flip) and a second GLWE; every TOY case here
    runs the K-split GEMM (atomics into zeroed rows). (7, 6) has beta L = 42:
    digits past 32 bits."""
    beta, lv, pk, rows = toy_packed
    _, ct = toy_inputs
    got = host_u64(toy.pack(dev_u64(toy, ct[:count]), count))
    assert got.shape == (-(-count // TOY.N), (TOY.k + 1) * TOY.N)
    want = R.pack_from_rows(rows[lv], ct, count, TOY.N)
    np.testing.assert_array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("count", [17, 300])
def test_pack_level_prefix_bit_exact_toy(toy, toy_inputs, toy_packed, count):
    beta, lv, pk, rows = toy_packed
    _, ct = toy_inputs
    for levels in (1, lv - 1, lv):
        got = host_u64(toy.pack(dev_u64(toy, ct[:count]), count, levels))
        want = R.pack_from_rows(rows[levels], ct, count, TOY.N)
        np.testing.assert_array_equal(got.reshape(want.shape), want)
    with pytest.raises(_lib.FheError, match="FHE_E_ARG"):
        toy.pack(dev_u64(toy, ct[:count]), count, lv + 1)


def test_pack_unsplit_gemm_bit_exact_toy(toy, toy_packed):
    """1100 inputs: 9 ciphertext blocks x 32 column blocks leave no room for a
    K split, so the GEMM stores instead of adding (the other GEMM path; the
    real-parameter cases below take it too); five GLWEs, the last partial."""
    beta, lv, pk, _ = toy_packed
    rng = np.random.default_rng(77)
    ct = rng.integers(0, 2 ** 64, (1100, toy.W), dtype=U)
    toy.profile(True)
    try:
        got = host_u64(toy.pack(dev_u64(toy, ct), 1100, 1))
        prof = toy.profile_read("pack")
    finally:
        toy.profile(False)
    assert prof["launches"] == 1 and prof["items"] == 1100 and prof["total_ms"] > 0
    assert toy.kernel_name("pack") == "k_keyswitch_mfma<8, 1>"
    want = R.pack_ref(ct, pk, beta, 1)
    np.testing.assert_array_equal(got.reshape(want.shape), want)


def key_noise(pk, s_big, p, beta, rows=None):
    """phase - message of key rows (all, or the given ones): int64 [rows, L, N]."""
    big, lv = pk.shape[:2]
    rows = np.arange(big) if rows is None else np.asarray(rows)
    ph = R.glwe_phase(pk[rows].reshape(-1, p.k + 1, p.N), s_big, p.N, p.k).reshape(len(rows), lv, p.N)
    with np.errstate(over="ignore"):
        for l in range(lv):
            ph[:, l, 0] -= s_big[rows] << U(64 - beta * (l + 1))
    return ph.astype(np.int64)


def check_key_noise(e, noise_bits):
    assert e.size >= 10 ** 5
    assert np.abs(e).max() <= 1 << noise_bits
    var = (2.0 ** (2 * noise_bits + 1) + 1.0) / 6.0
    assert 0.95 * var <= float(np.mean(e.astype(np.float64) ** 2)) <= 1.05 * var
    assert abs(e.mean()) < 0.02 * math.sqrt(var)


def test_pack_key_rows_toy(toy, toy_packed):
    beta, lv, pk, _ = toy_packed
    check_key_noise(key_noise(pk, s_big_of(toy), TOY, beta), TOY.glwe_noise_bits)


@pytest.fixture(scope="module")
def p16(need_gpu):
    p = params_for_bits(16)
    eng = Engine(p, 0)
    eng.keygen(7)
    beta, lv, _ = pack_plan(p, 1024, 0.0)
    eng.keygen_pack(beta, lv, seed=8)
    return eng


def test_pack_key_rows_p16(p16):
    p = p16.params
    beta, lv = p16.pack_gadget
    rows = np.arange(0, p.k * p.N, 51)                 # 41 rows x lv levels x 1024 coefficients
    e = key_noise(pack_key_of(p16), s_big_of(p16), p, beta, rows)
    check_key_noise(e, p.glwe_noise_bits)


@pytest.mark.parametrize("count", [1, 256, 257])
def test_decrypt_packed_modes_toy(toy, toy_packed, count):
    beta, lv, pk, _ = toy_packed
    P = TOY.msg_bits
    rng = np.random.default_rng(count)
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), count)
    msgs[:4][:count] = (-(1 << (P - 1)), (1 << (P - 1)) - 1, 0, -1)[:count]
    ends = rng.choice([-(1 << (P - 1)), 0], count)               # phases at 2^63 and 0: bits
    s_big = s_big_of(toy)
    for vals, modes in ((msgs, (0, 2)), (ends, (0, 1, 2))):
        ct = toy.encrypt(vals, seed=5 + count, id0=9)
        glwe = toy.pack(ct, count)
        phase = R.glwe_phase(host_u64(glwe), s_big, TOY.N, TOY.k).reshape(-1)[:count]
        for mode in modes:
            got = toy.decrypt_packed(glwe, count, mode).cpu().numpy()
            if mode == 2:
                np.testing.assert_array_equal(got.view(U), phase)
            elif mode == 1:
                np.testing.assert_array_equal(got, ((phase + U(1 << 62)) >> U(63)).astype(np.int64))
                np.testing.assert_array_equal(got, toy.decrypt_bits(ct).cpu().numpy())
                np.testing.assert_array_equal(got, (vals != 0).astype(np.int64))
            else:
                q = ((((phase >> U(63 - P)) + U(1)) >> U(1)) & U((1 << P) - 1)).astype(np.int64)
                np.testing.assert_array_equal(got, np.where(q >= 1 << (P - 1), q - (1 << P), q))
                # (4, 3) rounds the masks to 12 bits: sigma = sqrt(257 / 12) 2^52 against TOY's
                # half step 2^55 is 1.7 sigma, no gadget for 8-bit values (its bits are safe);
                # (7, 6) keeps 2^55 / sqrt(pack_var) > 2^20 sigma
                if (beta, lv) == (7, 6):
                    assert 2.0 ** (63 - P) / math.sqrt(R.pack_var(TOY, count, beta, lv)) > 1000
                    np.testing.assert_array_equal(got, toy.decrypt(ct).cpu().numpy())
                    np.testing.assert_array_equal(got, vals)
    with pytest.raises(_lib.FheError, match="FHE_E_ARG"):
        toy.decrypt_packed(glwe, count, 3)


def sampled_coefficients(ct, pk, beta, lv, samples, N):
    """The restatement's output at (component, coefficient) samples:
    count * kN * L multiply-adds each."""
    big, k = pk.shape[0], pk.shape[2] - 1
    count = len(ct)
    d = R.decompose_ks_np(ct[:, :big], beta, lv).astype(U)           # [count, big, lv]
    j = np.arange(count)
    out = []
    with np.errstate(over="ignore"):
        for c, t in samples:
            key = pk[:, :, c, (t - j) % N]                           # [big, lv, count]
            m = U(0) - np.einsum("jil,ilj->j", d, key)
            v = np.where(t >= j, m, U(0) - m).sum(dtype=U)
            if c == k and t < count:
                v += ct[t, big]
            out.append(v)
    return np.array(out, U)


@pytest.mark.parametrize("P", [16, 27])
def test_pack_real_parameters(need_gpu, p16, P):
    """P = 16 and P = 27 with their planned gadgets, 130 inputs (two 128-row
    workgroups; the unsplit GEMM path): sampled output words against the
    restatement and every decrypted value exact."""
    if P == 16:
        eng = p16
    else:
        eng = Engine(params_for_bits(P), 0)
        eng.keygen(21)
        eng.keygen_pack(*pack_plan(eng.params, 1024, 0.0)[:2], seed=22)
    p = eng.params
    beta, lv = eng.pack_gadget
    count = 130
    rng = np.random.default_rng(P)
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), count)
    msgs[:4] = (-(1 << (P - 1)), (1 << (P - 1)) - 1, 0, -1)
    ct_d = eng.encrypt(msgs, seed=31, id0=1)
    glwe = eng.pack(ct_d, count)
    np.testing.assert_array_equal(eng.decrypt_packed(glwe, count, 0).cpu().numpy(), msgs)
    np.testing.assert_array_equal(eng.decrypt(ct_d).cpu().numpy(), msgs)
    samples = [(c, t) for c in range(p.k + 1) for t in (0, 129, p.N - 1)]
    samples += [(int(c), int(t)) for c, t in zip(rng.integers(0, p.k + 1, 247), rng.integers(0, p.N, 247))]
    assert len(samples) >= 256
    want = sampled_coefficients(host_u64(ct_d).reshape(count, eng.W), pack_key_of(eng), beta, lv, samples, p.N)
    got = host_u64(glwe).reshape(p.k + 1, p.N)
    np.testing.assert_array_equal(np.array([got[c, t] for c, t in samples], U), want)
    if P != 16:
        eng.close()


def test_pack_noise_p16(p16):
    """4 GLWEs of 1024 inputs: the packing error (packed phase minus the
    input's phase) has the model's standard deviation within 0.9-1.1x (4096
    samples: the estimator's own sigma is 1.1%) and no outlier past 6 sigma."""
    p = p16.params
    beta, lv = p16.pack_gadget
    P = p.msg_bits
    count = 4 * p.N
    msgs = np.random.default_rng(3).integers(-(1 << (P - 1)), 1 << (P - 1), count)
    ct = p16.encrypt(msgs, seed=77, id0=5)
    glwe = p16.pack(ct, count)
    assert glwe.shape[0] == 4
    err = (host_u64(p16.decrypt_packed(glwe, count, 2)) - host_u64(p16.phase(ct))).astype(np.int64)
    sigma = math.sqrt(R.pack_var(p, 1024, beta, lv))
    print(f"pack noise P=16 ({beta},{lv}): std {err.std():.4g}, model {sigma:.4g}, ratio {err.std() / sigma:.3f}, "
          f"max {np.abs(err).max() / sigma:.2f} sigma")
    assert 0.9 * sigma <= err.std() <= 1.1 * sigma
    assert np.abs(err).max() <= 6 * sigma
    np.testing.assert_array_equal(p16.decrypt_packed(glwe, count, 0).cpu().numpy(), msgs)


def refused(fn, *a):
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*secret"):
        fn(*a)


def check_eval_only(B, ct):
    """B holds evaluation keys only: everything that needs the secret is FHE_E_STATE."""
    L = B._L
    refused(B.encrypt, [1, 2], 3)
    refused(B.decrypt, ct)
    refused(B.decrypt_bits, ct)
    refused(B.phase, ct)
    refused(B.sign_trace, ct.clone())
    refused(B.keygen_pack, 4, 3)
    refused(B.export_keys)
    refused(B.decrypt_packed, ct, 1, 0)
    key = B._key(np.arange(8, dtype=np.uint32))
    p = C.c_void_p(ct.data_ptr())
    assert L.fhe_compare_query_batch(B._ctx, p, 0, key, p, 2, 4, p, 0, 0, p, p, None) == -3
    assert b"secret" in L.fhe_last_error(B._ctx)
    assert L.fhe_compare_batch(B._ctx, p, 2, 4, p, 0, 0, 1, 0, p, p, None) == -3
    assert L.fhe_score_batch(B._ctx, p, 2, 4, p, 0, 0, 1, 0, p, None) == -3
    s = np.zeros(B.big, U)
    assert L.fhe_export_keys(B._ctx, None, C.c_void_p(s.ctypes.data), None, None) == -3
    assert not s.any()


def test_eval_only_context(toy, toy_packed, toy_inputs, tmp_path):
    from fheicp.query import load_eval_keys, save_eval_keys
    A = toy
    keys = A.export_eval_keys()
    assert set(keys) == {"bsk", "ksk", "pack_key", "pack_gadget"}        # TOY has no other gadget
    save_eval_keys(str(tmp_path / "eval.npz"), keys)
    loaded = load_eval_keys(str(tmp_path / "eval.npz"))
    msgs = toy_inputs[0][:40]
    ct = A.encrypt(msgs, seed=2, id0=50)
    want_sign = A.sign(ct.clone())
    want_pack = A.pack(ct, 40)
    np.testing.assert_array_equal(A.decrypt_bits(want_sign).cpu().numpy(), (msgs < 0).astype(np.int64))
    fresh = Engine(TOY, 0)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        fresh.sign(ct.clone())                                           # no keys at all yet
    had_keys = Engine(TOY, 0)
    had_keys.keygen(1234)
    assert had_keys.decrypt(had_keys.encrypt(msgs, seed=1)).cpu().numpy().tolist() == msgs.tolist()
    for B in (fresh, had_keys):
        B.import_eval_keys(loaded)
        check_eval_only(B, ct)
        # same keys, deterministic evaluation: word for word what A computes
        assert torch.equal(B.sign(ct.clone()), want_sign)
        assert torch.equal(B.pack(ct, 40), want_pack)
        assert torch.equal(B.keyswitch(ct), A.keyswitch(ct))
        assert torch.equal(B.threshold(ct, 3), A.threshold(ct, 3))
        again = B.export_eval_keys()
        for k in keys:
            np.testing.assert_array_equal(again[k], keys[k])
        B.close()
    # the key holder still works after handing the keys out
    np.testing.assert_array_equal(A.decrypt(ct).cpu().numpy(), msgs)


def test_eval_import_needs_every_present_gadget(p16):
    keys = p16.export_eval_keys()
    gadgets = [k for k in keys if k.startswith("gadget_bsk")]
    assert gadgets                                                       # P = 16 has fast gadgets
    B = Engine(p16.params, 0)
    short = {k: v for k, v in keys.items() if k != gadgets[-1]}
    with pytest.raises(_lib.FheError, match="FHE_E_ARG.*gadget"):
        B.import_eval_keys(short)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        B.keyswitch(p16.encrypt([1], seed=1))                            # the failed import left no keys
    B.import_eval_keys(keys)
    ct = p16.encrypt([5, -7, 0], seed=4)
    assert torch.equal(B.sign(ct.clone()), p16.sign(ct.clone()))
    B.close()


@pytest.fixture(scope="module")
def two_party(need_gpu, tmp_path_factory):
    """The 16-dim, n_bits 6 model of tests/test_gpu_query.py (P0 = 21): the
    client on the corpus context, the server from an .npz of evaluation keys."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.query import EncryptedQuerySearch, QueryClient, QueryServer, save_eval_keys
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    assert c.P0 == 21
    client = QueryClient(c, pack_seed=17)
    assert client.margin >= 9.2
    path = str(tmp_path_factory.mktemp("keys") / "eval.npz")
    keys = client.eval_keys()
    assert not {"s_small", "s_big"} & set(keys)
    save_eval_keys(path, keys)
    server = QueryServer.from_npz(path, cq, c.P0)
    return c, EncryptedQuerySearch(c), client, server, oq


@pytest.mark.parametrize("B", [40, 130])
def test_two_party_search_end_to_end(two_party, B):
    c, single, client, server, oq = two_party
    s_e = c.cq.s_e
    p = c.scheme
    q, docs = Q.make_corpus(16, B, seed=30 + B)
    ref_acc = Q.corpus_accumulate(oq, s_e, 6, q, docs)
    scores = np.float64(Q.corpus_out_scale(oq, s_e)) * ref_acc.astype(np.float64)
    payload = client.encrypt_query(q)
    docs8 = server.pack_docs(docs)
    for t in (0.5, float(np.median(scores))):
        want_below = (scores < t).astype(np.int64)
        reply = server.search(payload, docs8, B, t)
        assert reply.dtype == U and reply.size == 4 + 2 * -(-B // p.N) * (p.k + 1) * p.N
        acc, below = client.decrypt_reply(reply)
        np.testing.assert_array_equal(acc.cpu().numpy(), ref_acc)
        np.testing.assert_array_equal(below.cpu().numpy(), want_below)
        # the single-party compare on the key holder's context, unchanged by
        # the shared leveled helper: still the clear restatement
        acc1, below1 = single.compare(payload, single.pack_docs(docs), B, t)
        np.testing.assert_array_equal(acc1.cpu().numpy(), ref_acc)
        np.testing.assert_array_equal(below1.cpu().numpy(), want_below)
        ka, ki = client.top_k(acc, below, 5)
        ka1, ki1 = c.engine.topk(acc1, below1, 5)
        assert torch.equal(ka, ka1) and torch.equal(ki, ki1)
    assert 0.25 <= want_below.mean() <= 0.75                            # documents on both sides
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*secret"):
        server.engine.decrypt(server.engine.empty_big(1))


def test_reference_side_binding_two_party(need_gpu):
    """integration/fhe_gpu.py's two-party calls (numpy and ctypes only): the
    packed reply of fhe_search_query_batch decrypts to what
    fhe_compare_query_batch returns, on TOY at 12 bits with a planned gadget."""
    import sys
    from pathlib import Path
    from fheicp import LIB_PATH
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "integration"))
    from fhe_gpu import GpuCompare
    p = TOY.with_msg_bits(12)
    eng = GpuCompare(p.as_dict(), key_seed=31, lib_path=str(LIB_PATH), enc_seed=1)
    try:
        b, lv, lb = eng.keygen_pack(count=40, seed=32)
        assert (b, lv, lb) == pack_plan(p, 40, 0.0)
        rng = np.random.default_rng(9)
        B, D = 40, 5
        dq, qq, w = rng.integers(-8, 8, (B, D)), rng.integers(-8, 8, D), rng.integers(-3, 4, D)
        cst, T = 11, -20
        want = dq @ (w * qq) + cst                       # |acc - T| <= 5 * 8 * 8 * 3 + 31 < 2^11
        docs = eng.pack_docs(dq)
        mk, nk = np.arange(8, dtype=np.uint32) + 5, np.arange(8, dtype=np.uint32) + 77
        body, id0 = eng.encrypt_query(qq, mk, nk, id0=1234)
        acc1, below1 = eng.compare_query(body, id0, mk, docs, w, cst, T)
        ga, gb = eng.search_query(body, id0, mk, docs, w, cst, T, lb)
        assert ga.size == gb.size == (p.k + 1) * p.N
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
