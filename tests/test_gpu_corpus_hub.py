"""GPU: the group key switch and the stored-ciphertext hub.

fhe_keyswitch_group_batch on engines with their own keys: every tenant's rows
equal its own fhe_keyswitch_batch word for word (the sums are exact modulo
2^64 for every K split), across the 128-row block and 16-row digit-group
edges, with tenants sitting out, on the unsplit path and at the real P = 21
parameters; padding rows and a row past M keep their canary. CorpusHub end to
end on TOY and at P0 = 21, with key rotation inside the hub: replies equal
the tenant's own CorpusServer word for word and decrypt to the clear
restatement (quant_ref.corpus_accumulate)."""
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


class KsTenants:
    """Engines with their own keys and nmax random big LWE rows each (a key
    switch is defined on any words; random rows exercise every digit)."""

    def __init__(self, params, seeds, nmax):
        self.engines = []
        for s in seeds:
            e = Engine(params, 0)
            e.keygen(s)
            self.engines.append(e)
        self.W, self.Ws = self.engines[0].W, self.engines[0].Ws
        rng = np.random.default_rng(4321)
        self.rows = [rng.integers(0, 2 ** 64, (nmax, self.W), dtype=U) for _ in seeds]
        self.group = EngineGroup(self.engines)

    def close(self):
        self.group.close()
        for e in self.engines:
            e.close()

    def check(self, counts, shift, add_body):
        """The group call on counts against each tenant's own
        fhe_keyswitch_batch, with canaries in the padding rows of d_small and
        in 16 rows past M."""
        M, starts = group_rows(counts)
        dev = self.engines[0].device
        big = np.random.default_rng(99).integers(0, 2 ** 64, (max(M, 1), self.W), dtype=U)  # padding rows hold noise
        for t, (n, s) in enumerate(zip(counts, starts)):
            big[s:s + n] = self.rows[t][:n]
        d_big = torch.from_numpy(big[:M].view(np.int64).copy()).to(dev)
        out = torch.full((M + 16, self.Ws), SENT_I64, dtype=torch.int64, device=dev)
        self.group.keyswitch(d_big, counts, shift, add_body, out=out)
        torch.cuda.synchronize()
        got = host_u64(out)
        np.testing.assert_array_equal(host_u64(d_big), big[:M])      # the input is only read
        real = np.zeros(M, bool)
        for t, (n, s) in enumerate(zip(counts, starts)):
            real[s:s + n] = True
            if not n:
                continue
            eng = self.engines[t]
            own = eng.keyswitch(torch.from_numpy(self.rows[t][:n].view(np.int64).copy()).to(dev), shift, add_body)
            np.testing.assert_array_equal(got[s:s + n], host_u64(own).reshape(n, self.Ws),
                                          err_msg=f"tenant {t} of {counts} against its own key switch")
        assert (got[M:] == U(SENTINEL)).all(), "rows past M were written"
        assert (got[:M][~real] == U(SENTINEL)).all(), "padding rows were written"
        return got, starts


@pytest.fixture(scope="module")
def toy_ks(need_gpu):
    t = KsTenants(TOY, (99, 100, 101), 130)
    yield t
    t.close()


# TOY: n + 1 = 65 columns are 5 blocks of 16, padded to 6 for CB = 3: 2 column
# groups; K = kN * ks_level = 2048 is KB = 32 k-blocks, so the split rule
# S = max(1, min(KB / 4, 2 CUs / (blocks * 2))), 2 CUs = 512 on the MI355X,
# gives S = 8 for the 4 blocks of (130, 1, 17) and for the single block of
# (0, 5, 0).
@pytest.mark.parametrize("shift,add_body", [(0, 0), (3, 0x0123456789ABCDEF)])
def test_group_keyswitch_block_and_digit_group_edges(toy_ks, shift, add_body):
    """130 rows: two ciphertext blocks, the second with one digit group of two
    rows; 1 row; 17 rows: two digit groups, the second with one row."""
    got, starts = toy_ks.check((130, 1, 17), shift, add_body)
    assert starts == [0, 132, 136] and got.shape[0] == 156 + 16
    # different keys: the same input row does not give the same words
    dev = toy_ks.engines[0].device
    row = torch.from_numpy(toy_ks.rows[0][:1].view(np.int64).copy()).to(dev)
    a, b = (host_u64(e.keyswitch(row.clone(), shift, add_body)) for e in toy_ks.engines[:2])
    assert not np.array_equal(a, b)


def test_group_keyswitch_tenants_sit_out(toy_ks):
    got, starts = toy_ks.check((0, 5, 0), 0, 0)
    assert starts == [0, 0, 8]
    toy_ks.check((0, 0, 0), 0, 0)


def test_group_keyswitch_profile_names_the_group_kernel(toy_ks):
    eng = toy_ks.engines[0]
    eng.profile(True)
    try:
        # tenant 0 sits out, so check() runs no key switch of its own on this engine: the bucket
        # (tenant 0's, as for the group rotations) holds the group launch pair alone
        toy_ks.check((0, 130, 17), 0, 0)
        prof = eng.profile_read("keyswitch")
    finally:
        eng.profile(False)
    assert eng.kernel_name("keyswitch") == "k_keyswitch_mfma_grp<3, 3>", eng.kernel_name("keyswitch")
    assert prof["launches"] == 1 and prof["items"] == 147 and prof["total_ms"] > 0


def test_group_keyswitch_unsplit_path(need_gpu):
    """S = 1: three tenants of 11,000 rows are 3 * ceil(11000 / 128) = 258
    ciphertext blocks, times TOY's 2 column groups 516 tiles; 512 / 516 = 0
    (512: two workgroups for each of the MI355X's 256 CUs),
    so the rule's max(1, .) leaves the K range whole and the GEMM stores
    instead of adding atomically (no zeroing by the digits kernel)."""
    t = KsTenants(TOY, (7, 8, 9), 11000)
    try:
        counts = (11000, 10999, 10993)
        assert sum(-(-n // 128) for n in counts) * 2 > 512
        t.check(counts, 2, 0xFEDCBA9876543210)
    finally:
        t.close()


def test_group_keyswitch_real_parameters_p21(need_gpu):
    t = KsTenants(params_for_bits(21), (99, 100), 3)
    try:
        t.check((3, 2), 0, 0)
        t.check((3, 2), 5, 1 << 40)
    finally:
        t.close()


def test_group_keyswitch_device_refusals(toy_ks):
    L, grp = toy_ks.group._L, toy_ks.group
    x = torch.zeros(8 * 513, dtype=torch.int64, device=toy_ks.engines[0].device)
    p = C.c_void_p(x.data_ptr())
    c = (C.c_int64 * 3)(1, 1, 1)
    assert L.fhe_keyswitch_group_batch(grp._grp, None, c, 0, 0, p, None) == -1
    assert b"null keyswitch buffers" in L.fhe_last_error(None)
    assert L.fhe_keyswitch_group_batch(grp._grp, p, c, 44, 0, p, None) == -1    # TOY's bound is 63 - 4 * 5 = 43
    assert b"shift" in L.fhe_last_error(None)
    z = (C.c_int64 * 3)(0, 0, 0)
    assert L.fhe_keyswitch_group_batch(grp._grp, None, z, 0, 0, None, None) == 0
    # the launch limits hold over all tenants together and are refused before any work is queued (the
    # buffers are never touched): 2 x ceil(600000 / 128) = 9376 blocks > 8191, each tenant alone below it
    big = (C.c_int64 * 3)(600000, 600000, 0)
    assert L.fhe_keyswitch_group_batch(grp._grp, p, big, 0, 0, p, None) == -1
    assert b"split the call" in L.fhe_last_error(None)
    assert L.fhe_sign_group_batch(grp._grp, p, big, p, None) == -1
    assert b"split the call" in L.fhe_last_error(None)


def test_group_corpus_argument_order(toy_ks):
    """FHE_E_ARG first, naming the tenant, then FHE_E_STATE: these engines
    hold no packing key, so every valid call ends at the key check, and every
    argument error must come before it. A group call's counts come before its
    shift bound."""
    L, grp = toy_ks.group._L, toy_ks.group
    x = torch.zeros(4096, dtype=torch.int64, device=toy_ks.engines[0].device)
    p = x.data_ptr()
    key = (C.c_uint32 * 8)()
    hT = (C.c_int64 * 2)(0, 0)

    def items(sizes, Qs, B_old=(0, 0, 0), B=4):
        arr = (_lib.FheGroupCorpus * 3)()
        for t in range(3):
            a = arr[t]
            a.struct_size, a.D, a.Q, a.B, a.B_old = sizes[t], 5, Qs[t], B, B_old[t]
            a.d_body = a.d_id0 = a.d_W = a.d_glwe_acc = a.d_glwe_bit = p
            a.h_mask_key, a.h_T = C.addressof(key), C.addressof(hT)
        return arr
    ok = C.sizeof(_lib.FheGroupCorpus)
    err = lambda: L.fhe_last_error(None)  # noqa: E731
    search = lambda a, T=3: L.fhe_search_seeded_queries_group_batch(grp._grp, a, T, None)  # noqa: E731
    assert search(items((ok, ok - 8, ok), (1, 1, 1))) == -1 and b"tenant 1" in err() and b"struct_size" in err()
    assert search(items((ok,) * 3, (1, 1, 2), B_old=(0, 0, 5))) == -1 and b"tenant 2" in err() and b"B_old" in err()
    assert search(items((ok,) * 3, (1, 1, 1), B_old=(-1, 0, 0))) == -1 and b"tenant 0" in err()
    a = items((ok,) * 3, (1, 1, 1))
    a[1].h_T = None
    assert search(a) == -1 and b"tenant 1" in err() and b"null" in err()
    a = items((ok,) * 3, (1, 1, 1))
    a[2].levels_bit = 9
    assert search(a) == -1 and b"tenant 2" in err() and b"levels_bit" in err()
    a = items((ok,) * 3, (1, 1, 1), B=2 ** 30)
    for t in range(3):
        a[t].D = 1
    assert search(a) == -1 and b"2^31" in err()
    assert search(items((ok,) * 3, (1, 1, 1)), T=2) == -1
    assert search(items((ok,) * 3, (0, -1, 0))) == -1 and b"tenant 1" in err()
    # valid arguments: the participating tenant without a packing key, by name; one sitting out is not asked
    assert search(items((ok,) * 3, (0, 1, 0))) == -3 and b"tenant 1" in err() and b"packing key" in err()
    assert search(items((ok, ok, ok), (0, 0, 0), B_old=(9, 9, 9))) == 0
    c = (C.c_int64 * 3)(1, 1, 1)
    assert L.fhe_keyswitch_group_batch(grp._grp, C.c_void_p(p), None, 44, 0, C.c_void_p(p), None) == -1
    assert b"counts" in err()
    assert L.fhe_keyswitch_group_batch(grp._grp, None, c, 44, 0, None, None) == -1 and b"shift" in err()


# ------------------------------------------------------------- CorpusHub --
def restate(oq, cq, n_e, queries, docs, ts):
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_e, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    below = np.stack([(scores[i] < t).astype(np.int64) if t is not None else np.zeros(len(docs), np.int64)
                      for i, t in enumerate(ts)])
    return ref, below, scores


def toy_model():
    """The 5-feature, 2-bit model of tests/test_gpu_group.py (P0 = 8)."""
    from fheicp.corpus import CorpusQuant
    from fheicp.model import QuantParams
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    return CorpusQuant(qp, 2, 0.5), Q.QuantizedLinearParams.from_json(qp.to_dict())


def check_hub(hub, tenants, requests, same_words=True):
    """tenants: {name: (client, oq, cq, n_e, queries, docs, ts)}. The hub's
    replies decrypt to the restatement with the tenant's client and, where the
    widths agree, equal the tenant's own server's word for word."""
    got = hub.search_many(requests)
    assert list(got) == list(requests)
    # before the tenants' own servers run: the key switch the hub's sign extraction launched (tenant 0's bucket)
    hub.ks_kernel = next(iter(hub.tenants.values())).engine.kernel_name("keyswitch")
    for name in requests:
        client, oq, cq, n_e, queries, docs, ts = tenants[name]
        ref, below, _ = restate(oq, cq, n_e, queries, docs, ts)
        acc, bits = client.decrypt_replies(got[name])
        np.testing.assert_array_equal(acc.cpu().numpy(), ref, err_msg=name)
        np.testing.assert_array_equal(bits.cpu().numpy(), below, err_msg=name)
        own = hub.tenants[name].search_many(queries, ts)
        acc, bits = client.decrypt_replies(own)
        np.testing.assert_array_equal(acc.cpu().numpy(), ref, err_msg=name)
        assert len(own) == len(got[name])
        for a, b in zip(got[name], own):
            pa, pb = int(a[1]) >> 32, int(b[1]) >> 32       # the replies' width fields
            assert pa >= pb
            if pa == pb and same_words:
                np.testing.assert_array_equal(a, b, err_msg=f"{name}: reply words against its own server")
    return got


@pytest.fixture(scope="module")
def toy_hub(need_gpu):
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusHub
    cq, oq = toy_model()
    hub, tenants = CorpusHub(0), {}
    for i, (name, (Qn, B)) in enumerate({"alice": (3, 130), "bob": (1, 1), "carol": (2, 17)}.items()):
        c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=99 + i, device=0, noise_seed=6 + i)
        assert c.P0 == 8
        client = CorpusClient(c, count=TOY.N, pack_seed=17 + i)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, c.mask_key, scheme=c.scheme)
        rng = np.random.default_rng(77 + i)
        qs = rng.uniform(-1.2, 0.7, (Qn, 5)).astype(np.float32)
        docs = rng.uniform(-1.2, 0.7, (B, 5)).astype(np.float32)
        assert hub.load(name, *client.encrypt_docs(docs)) == B
        scores = restate(oq, cq, 2, qs, docs, [None] * Qn)[2]
        med = float(np.median(scores[Qn // 2]))
        ts = {"alice": [None, med, 0.5], "bob": [0.5], "carol": [None, med]}[name]
        tenants[name] = (client, oq, cq, 2, qs, docs, ts)
    return hub, tenants


def test_corpus_hub_toy_end_to_end(toy_hub):
    hub, tenants = toy_hub
    requests = {name: (t[4], t[6]) for name, t in tenants.items()}
    rounds = hub.rounds(requests)
    assert [r["mode"] for r in rounds] == ["group"] and len(rounds[0]["parts"]) == 3
    got = check_hub(hub, tenants, requests)
    assert hub.ks_kernel == "k_keyswitch_mfma_grp<3, 3>", hub.ks_kernel
    # both bit values occur for the median rows
    for name, row in (("alice", 1), ("carol", 1)):
        client, oq, cq, n_e, qs, docs, ts = tenants[name]
        below = restate(oq, cq, n_e, qs, docs, ts)[1]
        assert 0 < below[row].sum() < len(docs), name
    # these seeds plan carol at the round's width (her words were compared with her own server's) and
    # alice and bob one bit below it: their rows ran shifted, above their own width, on the device
    P = rounds[0]["P"]
    assert P == 7 and {p["name"]: p["P_t"] for p in rounds[0]["parts"]} == {"alice": 6, "bob": 6, "carol": 7}
    assert all(int(r[1]) >> 32 == P for rs in got.values() for r in rs)
    # a tenant sitting out changes nothing for the others
    part = hub.search_many({n: requests[n] for n in ("alice", "carol")})
    r2 = hub.rounds({n: requests[n] for n in ("alice", "carol")})
    assert [r["mode"] for r in r2] == ["group"] and r2[0]["P"] == P     # the same width without bob
    for n in ("alice", "carol"):
        np.testing.assert_array_equal(part[n][0], got[n][0], err_msg=f"{n}: reply words with bob sitting out")
    for n in ("alice", "carol"):
        acc, _ = tenants[n][0].decrypt_replies(part[n])
        np.testing.assert_array_equal(acc.cpu().numpy(), restate(*tenants[n][1:])[0])
    # a tenant alone goes through its own server
    only = hub.search_many({"carol": requests["carol"]})
    own = hub.tenants["carol"].search_many(*requests["carol"])
    np.testing.assert_array_equal(only["carol"][0], own[0])
    # another tenant's client does not open a reply
    acc, _ = tenants["alice"][0].decrypt_replies(got["carol"])
    assert not np.array_equal(acc.cpu().numpy(), restate(*tenants["carol"][1:])[0])


def test_corpus_hub_rotation_inside_the_hub(need_gpu):
    """One call with alice rekeyed (every document old), bob rekeyed and then
    appended to (half old) and carol never rotated."""
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusHub
    cq, oq = toy_model()
    hub, tenants, old_clients = CorpusHub(0), {}, {}
    rng = np.random.default_rng(5)
    queries = rng.uniform(-1.2, 0.7, (2, 5)).astype(np.float32)
    for i, (name, B) in enumerate({"alice": 12, "bob": 10, "carol": 7}.items()):
        c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=50 + i, device=0, noise_seed=60 + i)
        client = CorpusClient(c, count=TOY.N, pack_seed=70 + i)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, c.mask_key, scheme=c.scheme)
        docs = rng.uniform(-1.2, 0.7, (B, 5)).astype(np.float32)
        scores = restate(oq, cq, 2, queries, docs, [None, None])[2]
        ts = [float(np.median(scores[0])), None]
        if name == "alice":
            hub.load(name, *client.encrypt_docs(docs))
            old_clients[name] = client
            client = client.rotate(key_seed=80, pack_seed=81, bridge_seed=82, noise_seed=83)
            hub.rekey(name, client.eval_keys())
            assert hub.tenants[name].b_old == 12
        elif name == "bob":
            hub.load(name, *client.encrypt_docs(docs[:5]))
            old_clients[name] = client
            client = client.rotate(key_seed=84, pack_seed=85, bridge_seed=86, noise_seed=87)
            hub.rekey(name, client.eval_keys())
            assert hub.append(name, *client.encrypt_docs(docs[5:])) == 10 and hub.tenants[name].b_old == 5
        else:
            hub.load(name, *client.encrypt_docs(docs))
        tenants[name] = (client, oq, cq, 2, queries, docs, ts)
    requests = {name: (t[4], t[6]) for name, t in tenants.items()}
    assert [r["mode"] for r in hub.rounds(requests)] == ["group"]
    got = check_hub(hub, tenants, requests)
    # the rotated-out key holders cannot open the new replies
    for name, old in old_clients.items():
        acc, _ = old.decrypt_replies(got[name])
        assert not np.array_equal(acc.cpu().numpy(), restate(*tenants[name][1:])[0]), name
    # B_old > 0 without a bridge key: FHE_E_STATE naming the tenant
    hub.tenants["carol"].b_old = 3
    try:
        with pytest.raises(_lib.FheError, match="FHE_E_STATE.*tenant 2.*bridge key"):
            hub.search_many(requests)
    finally:
        hub.tenants["carol"].b_old = 0


def test_corpus_hub_real_parameters_p21(need_gpu):
    """The 16-dim, n_bits 6 model (P0 = 21): two tenants, (Q, B) = (1, 5) and
    (2, 3), the first rotated with 3 of its 5 documents old."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.stored import CorpusClient, CorpusHub
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    hub, tenants = CorpusHub(0), {}
    for i, (name, (Qn, B)) in enumerate({"alice": (1, 5), "bob": (2, 3)}.items()):
        c = EncryptedCorpus(cq).compile(key_seed=5 + i, device=0, noise_seed=6 + i)
        assert c.P0 == 21
        client = CorpusClient(c, pack_seed=17 + i)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, c.mask_key)
        qs, docs = [], None
        for j in range(Qn):
            q, d = Q.make_corpus(16, B, seed=40 + 10 * i + j)
            qs.append(q)
            docs = d if docs is None else docs
        if name == "alice":
            hub.load(name, *client.encrypt_docs(docs[:3]))
            client = client.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
            hub.rekey(name, client.eval_keys())
            hub.append(name, *client.encrypt_docs(docs[3:]))
            assert hub.tenants[name].b_old == 3
        else:
            hub.load(name, *client.encrypt_docs(docs))
        ts = [0.5] if Qn == 1 else [None, 0.5]
        tenants[name] = (client, oq, cq, 6, np.stack(qs), docs, ts)
    requests = {name: (t[4], t[6]) for name, t in tenants.items()}
    assert [r["mode"] for r in hub.rounds(requests)] == ["group"]
    check_hub(hub, tenants, requests)
    assert hub.ks_kernel == "k_keyswitch_mfma_grp<3, 3>", hub.ks_kernel
