"""GPU: several key holders in one batched call.

Three TOY engines with key seeds 99, 100, 101: the group sign extraction over
the padded row layout equals, word for word, fhe_sign_batch on each tenant's
own engine, leaves padding and trailing rows alone, and a tenant's words do
not depend on who shares the launch or in which order. End to end through
QueryHub on TOY and on the real P0 = 21 parameters every reply equals the
tenant's own QueryServer.search_many word for word and decrypts to the clear
restatement (quant_ref.corpus_accumulate); P = 26 runs the deep multi-bit
kernels' group forms."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine, EngineGroup, group_rows
from fheicp.params import TOY, params_for_bits

pytestmark = pytest.mark.gpu

U = np.uint64
SENTINEL = 0x5EA15EA15EA15EA1
SENT_I64 = int(np.array(SENTINEL, U).view(np.int64))


def host_u64(t):
    return t.cpu().numpy().view(U)


def values(P, n, seed):
    """n >= 4 values on both sides of zero; -1, 0 and +-(2^(P-1) - 1) lead."""
    top = 2 ** (P - 1) - 1
    rng = np.random.default_rng(seed)
    return np.concatenate([[-1, 0, top, -top], rng.integers(-top, top + 1, n - 4)]).astype(np.int64)


def group_sign_raw(grp, ctv, counts, sign):
    """fhe_sign_group_batch on the caller's buffers (the canary needs its own)."""
    c = (C.c_int64 * len(counts))(*counts)
    rc = grp._L.fhe_sign_group_batch(grp._grp, C.c_void_p(ctv.data_ptr()), c, C.c_void_p(sign.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream(grp.device).cuda_stream))
    _lib.check(rc)
    torch.cuda.synchronize()


class Tenants:
    """Engines with their own keys, encryptions of `values` under each key and
    each tenant's own fhe_sign_batch of them, computed once."""

    def __init__(self, params, seeds, nmax):
        self.engines = []
        for s in seeds:
            e = Engine(params, 0)
            e.keygen(s)
            self.engines.append(e)
        P = params.msg_bits
        self.vals = [values(P, nmax, 7 + t) for t in range(len(seeds))]
        self.cts = [e.encrypt(v, seed=31 + t, id0=5) for t, (e, v) in enumerate(zip(self.engines, self.vals))]
        self.own = [host_u64(e.sign(ct.clone())).reshape(nmax, e.W).copy() for e, ct in zip(self.engines, self.cts)]
        self.group = EngineGroup(self.engines)
        self.W = self.engines[0].W

    def run(self, counts, order=None, group=None):
        """The group call on counts (tenant order `order`): (ct_v before, ct_v
        after, the sign buffer of M + 16 rows, starts), host u64 arrays."""
        order = list(range(len(counts))) if order is None else order
        M, starts = group_rows(counts)
        dev = self.engines[0].device
        rng = np.random.default_rng(1234)
        before = rng.integers(0, 2 ** 64, (M, self.W), dtype=U)        # padding rows hold noise
        for t, n, s in zip(order, counts, starts):
            before[s:s + n] = host_u64(self.cts[t]).reshape(-1, self.W)[:n]
        ctv = torch.from_numpy(before.view(np.int64).copy()).to(dev)
        sign = torch.full((M + 16, self.W), SENT_I64, dtype=torch.int64, device=dev)
        group_sign_raw(group or self.group, ctv, counts, sign)
        return before, host_u64(ctv), host_u64(sign), starts


@pytest.fixture(scope="module")
def toy3(need_gpu):
    t = Tenants(TOY, (99, 100, 101), 6)
    t.first = t.run((5, 1, 6))
    return t


def check_against_own(t, counts, sign, starts, order=None):
    order = list(range(len(counts))) if order is None else order
    for tt, n, s in zip(order, counts, starts):
        np.testing.assert_array_equal(sign[s:s + n], t.own[tt][:n], err_msg=f"tenant {tt} against its own sign batch")
        if n:
            eng = t.engines[tt]
            rows = torch.from_numpy(sign[s:s + n].view(np.int64).copy()).to(eng.device)
            np.testing.assert_array_equal(eng.decrypt_bits(rows).cpu().numpy(), (t.vals[tt][:n] < 0).astype(np.int64))


def test_group_sign_equals_each_tenants_own(toy3):
    counts = (5, 1, 6)
    _, _, sign, starts = toy3.first
    assert starts == [0, 8, 12] and sign.shape[0] == 20 + 16
    for v in toy3.vals:
        assert {-1, 0, 127, -127} <= set(v.tolist()) and (v < 0).any() and (v > 0).any()
    check_against_own(toy3, counts, sign, starts)
    # different keys: the same plaintext rows do not give the same words
    assert not np.array_equal(toy3.own[0][0], toy3.own[1][0])


def test_group_sign_canary(toy3):
    counts = (5, 1, 6)
    before, after, sign, starts = toy3.first
    M = before.shape[0]
    real = np.zeros(M, bool)
    for n, s in zip(counts, starts):
        real[s:s + n] = True
    assert real.sum() == 12 and (~real).sum() == 8
    assert (sign[M:] == U(SENTINEL)).all()                       # the 16 trailing rows
    assert (sign[:M][~real] == U(SENTINEL)).all()                # padding rows of the sign buffer
    np.testing.assert_array_equal(after[~real], before[~real])    # ... and of ct_v
    assert not (sign[:M][real] == U(SENTINEL)).all(axis=1).any()  # every real row was written
    assert (after[real] != before[real]).any(axis=1).all()        # ct_v is consumed


@pytest.mark.parametrize("counts", [(4, 0, 1), (1, 1, 1), (0, 0, 3), (0, 0, 0)])
def test_group_sign_edges(toy3, counts):
    before, after, sign, starts = toy3.run(counts)
    M = before.shape[0]
    assert M == sum(-(-n // 4) * 4 for n in counts)
    check_against_own(toy3, counts, sign, starts)
    assert (sign[M:] == U(SENTINEL)).all()
    real = np.zeros(M, bool)
    for n, s in zip(counts, starts):
        real[s:s + n] = True
    assert (sign[:M][~real] == U(SENTINEL)).all()
    np.testing.assert_array_equal(after[~real], before[~real])


def test_group_of_one_equals_sign_batch(toy3):
    g1 = EngineGroup([toy3.engines[1]])
    for n in (6, 5):
        M, starts = group_rows([n])
        ctv = torch.zeros((M, toy3.W), dtype=torch.int64, device=toy3.engines[1].device)
        ctv[:n] = toy3.cts[1][:n]
        sign = g1.sign(ctv, [n])
        np.testing.assert_array_equal(host_u64(sign)[:n], toy3.own[1][:n])
    g1.close()


def test_group_sign_independent_of_company_and_order(toy3):
    with_others = toy3.first[2][:5]
    _, _, alone, starts = toy3.run((5, 0, 0))
    assert starts == [0, 8, 8]
    np.testing.assert_array_equal(alone[:5], with_others)
    rev = EngineGroup(toy3.engines[::-1])
    _, _, sign, starts = toy3.run((6, 1, 5), order=[2, 1, 0], group=rev)
    assert starts == [0, 8, 12]
    np.testing.assert_array_equal(sign[12:17], with_others)
    check_against_own(toy3, (6, 1, 5), sign, starts, order=[2, 1, 0])
    rev.close()


def test_group_rejections_on_the_device(toy3):
    """The TOY engines hold no packing key: a participating tenant is
    FHE_E_STATE from the search entry (a tenant that sits out is not asked);
    a stale struct_size is an argument error, reported first."""
    L, grp = toy3.group._L, toy3.group
    x = torch.zeros(4096, dtype=torch.int64, device=toy3.engines[0].device)
    p = x.data_ptr()
    key = (C.c_uint32 * 8)()
    hT = (C.c_int64 * 1)(0)

    def items(size, Qs):
        arr = (_lib.FheGroupQuery * 3)()
        for t in range(3):
            arr[t].struct_size = size
            arr[t].D, arr[t].Q, arr[t].B = 1, Qs[t], 1
            arr[t].d_qbody = arr[t].d_id0 = arr[t].d_docs8 = arr[t].d_w = arr[t].d_glwe_acc = arr[t].d_glwe_bit = p
            arr[t].h_mask_key, arr[t].h_T = C.addressof(key), C.addressof(hT)
        return arr
    ok = C.sizeof(_lib.FheGroupQuery)
    assert L.fhe_search_query_group_batch(grp._grp, items(ok, (0, 1, 0)), 3, None) == -3
    assert b"packing key" in L.fhe_last_error(None)
    assert L.fhe_search_query_group_batch(grp._grp, items(ok, (0, 0, 0)), 3, None) == 0
    assert L.fhe_search_query_group_batch(grp._grp, items(ok - 8, (0, 1, 0)), 3, None) == -1
    assert b"struct_size" in L.fhe_last_error(None)
    assert L.fhe_search_query_group_batch(grp._grp, items(ok, (0, 1, 0)), 2, None) == -1
    assert L.fhe_search_query_group_batch(grp._grp, items(ok, (0, -1, 0)), 3, None) == -1
    # a tenant whose width moved away from the others' is refused at the call
    toy3.engines[2].set_msg_bits(12)
    try:
        c = (C.c_int64 * 3)(1, 1, 1)
        assert L.fhe_sign_group_batch(grp._grp, C.c_void_p(p), c, C.c_void_p(p), None) == -1
        assert b"tenant 2" in L.fhe_last_error(None)
    finally:
        toy3.engines[2].set_msg_bits(TOY.msg_bits)
    # a group across a keyless engine: FHE_E_STATE at creation
    bare = Engine(TOY, 0)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*tenant 1"):
        EngineGroup([toy3.engines[0], bare])
    bare.close()


# ---------------------------------------------------------- through QueryHub --
def hub_case(hub, tenants):
    """tenants: {name: (client, cq, oq, n_e, qs, docs, ts)}. Runs the hub and
    every tenant's own server; checks replies word for word, decrypted values
    against the clear restatement."""
    requests, want = {}, {}
    for name, (client, cq, oq, n_e, qs, docs, ts) in tenants.items():
        B = hub.load(name, docs)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_e, q, docs) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        below = np.stack([np.zeros(B, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                          for q, t in enumerate(ts)])
        requests[name] = (client.encrypt_queries(qs), ts)
        want[name] = (ref, below)
    got = hub.search_many(requests)
    assert list(got) == list(requests)
    for name, (client, *_rest) in tenants.items():
        rec = hub.tenants[name]
        own = rec["server"].search_many(requests[name][0], rec["docs8"], rec["B"], requests[name][1])
        assert len(got[name]) == len(own) == 1
        np.testing.assert_array_equal(got[name][0], own[0], err_msg=f"{name}: reply words against its own server")
        for replies in (got[name], own):
            acc, below = client.decrypt_replies(replies)
            np.testing.assert_array_equal(acc.cpu().numpy(), want[name][0], err_msg=name)
            np.testing.assert_array_equal(below.cpu().numpy(), want[name][1], err_msg=name)
    return want


def test_hub_toy_end_to_end(need_gpu):
    """The 5-feature, 2-bit model of tests/test_gpu_multi_query.py (P0 = 8):
    three tenants with their own keys, (Q, B) = (3, 130), (1, 1), (2, 17)."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.model import QuantParams
    from fheicp.query import QueryClient, QueryHub
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    cq = CorpusQuant(qp, 2, 0.5)
    oq = Q.QuantizedLinearParams.from_json(qp.to_dict())
    hub, tenants = QueryHub(0), {}
    shapes = {"alice": (3, 130), "bob": (1, 1), "carol": (2, 17)}
    for i, (name, (Qn, B)) in enumerate(shapes.items()):
        c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=99 + i, device=0, noise_seed=6 + i)
        assert c.P0 == 8
        client = QueryClient(c, count=TOY.N, pack_seed=17 + i)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, scheme=c.scheme)
        rng = np.random.default_rng(77 + i)
        qs = rng.uniform(-1.2, 0.7, (Qn, 5)).astype(np.float32)
        docs = rng.uniform(-1.2, 0.7, (B, 5)).astype(np.float32)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 2, q, docs) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        # thresholds: None, a median (both outcomes occur, asserted below), a fixed one
        med = float(np.median(scores[Qn // 2]))
        ts = {"alice": [None, med, 0.5], "bob": [0.5], "carol": [None, med]}[name]
        tenants[name] = (client, cq, oq, 2, qs, docs, ts)
    with pytest.raises(ValueError, match="'dave'.*P0"):
        hub.add_tenant("dave", {}, cq, 12, scheme=TOY)
    want = hub_case(hub, tenants)
    assert 0 < want["alice"][1][1].sum() < 130 and 0 < want["carol"][1][1].sum() < 17
    # one tenant alone goes through its own server; one sitting out changes nothing
    only = hub.search_many({"carol": (tenants["carol"][0].encrypt_queries(tenants["carol"][4]), None)})
    acc, _ = tenants["carol"][0].decrypt_replies(only["carol"])
    np.testing.assert_array_equal(acc.cpu().numpy(), want["carol"][0])


def test_hub_real_parameters_p21(need_gpu):
    """The 16-dim, n_bits 6 model (P0 = 21), two tenants with different keys,
    (Q, B) = (1, 5) and (2, 3): the group forms of mb64<4>, mb64<3>,
    mb<2,0,15> and mb<1,0,23>."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.query import QueryClient, QueryHub
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    hub, tenants = QueryHub(0), {}
    for i, (name, (Qn, B)) in enumerate({"alice": (1, 5), "bob": (2, 3)}.items()):
        c = EncryptedCorpus(cq).compile(key_seed=5 + i, device=0, noise_seed=6 + i)
        assert c.P0 == 21
        client = QueryClient(c, pack_seed=17 + i)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0)
        qs, docs = [], None
        for j in range(Qn):
            q, d = Q.make_corpus(16, B, seed=40 + 10 * i + j)
            qs.append(q)
            docs = d if docs is None else docs
        ts = [0.5] if Qn == 1 else [None, 0.5]
        tenants[name] = (client, cq, oq, 6, np.stack(qs), docs, ts)
    hub_case(hub, tenants)


def test_group_sign_real_parameters_p26(need_gpu):
    """P = 26: the group forms of the deep multi-bit kernels (mb64<8> and
    mb64<5> among them), two tenants, counts (3, 2): bits exact and the words
    those of each tenant's own fhe_sign_batch."""
    p = params_for_bits(26)
    t = Tenants(p, (99, 100), 4)
    eng = t.engines[0]
    counts = (3, 2)
    _, _, sign, starts = t.run(counts)
    ran = {eng.kernel_name(k) for k in ("blind_rotate_main", "blind_rotate_fast", "blind_rotate_fast2",
                                        "blind_rotate_mid", "blind_rotate_mid2", "blind_rotate_mid0")}
    assert {"k_blind_rotate_mb64_grp<8>", "k_blind_rotate_mb64_grp<5>"} <= ran, ran
    assert all("_grp<" in n for n in ran if n)
    check_against_own(t, counts, sign, starts)
    for v in t.vals:
        assert {-1, 0, 2 ** 25 - 1, -(2 ** 25 - 1)} == set(v.tolist())
