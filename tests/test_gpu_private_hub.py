"""GPU: the both-private search for several key holders.

Three TOY engines with their own keys, each with its own GGSW queries and its
own document GLWEs (made as in tests/test_gpu_private_queries.py: GPU-made
GGSWs with the edge words planted, arbitrary GLWE words with the tie inputs).
The grouped leveled step (fhe_linear_ggsws_group_batch: one table launch, one
plane launch, one grouped transposed external product, one extraction) equals
each tenant's own fhe_linear_ggsws_batch and the numpy restatement
(tests/extprod_ref.py) word for word over the padded group layout, leaves
padding rows and the rows past M alone, and a tenant's words depend neither on
who shares the launch nor on the order. End to end through PrivateHub on TOY
and on the real P0 = 21 parameters every reply equals the tenant's own
PrivateServer.search_many word for word and decrypts to the clear restatement
(quant_ref.corpus_accumulate)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import extprod_ref as X
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine, EngineGroup, group_rows, u64
from fheicp.params import TOY

pytestmark = pytest.mark.gpu

U = np.uint64
GADGETS = [(4, 3), (7, 7)]
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0, 1 << 63)
QMAX, GMAX = 11, 17
CSTS = [-37, 5, 0, 11, -1, 300, -4096, 2, 7, -8, 1]
SENT = -0x0123456789ABCDEF
E_ARG = -1


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(eng.device)


def shape(p, G, D):
    """B of G GLWEs of D-feature documents, the last GLWE partly filled."""
    S = p.N // D
    return G * S if S == 1 else (G - 1) * S + max(1, S // 3)


class Tenants:
    """Three engines with their own keys; per (tenant, gadget) QMAX GGSWs and
    GMAX document GLWEs of its own, on the host and on the device."""

    def __init__(self):
        self.engines = []
        for s in (99, 100, 101):
            e = Engine(TOY, 0)
            e.keygen(s)
            self.engines.append(e)
        self.group = EngineGroup(self.engines)
        self.p = p = TOY
        self.W = self.engines[0].W
        self.host, self.dev = {}, {}
        for t, eng in enumerate(self.engines):
            for beta, L in GADGETS:
                rng = np.random.default_rng(1000 * t + 200 * beta + L)
                ggsws = []
                for q in range(QMAX):
                    Wt = rng.integers(-2 ** 12, 2 ** 12, 16)
                    Wt[q % 16] = 0
                    g = u64(eng.encrypt_ggsw(Wt, beta, L, 77 + q + 50 * t, id0=1000 * q)).reshape(
                        p.k + 1, L, p.k + 1, p.N).copy()
                    for i, w in enumerate(EDGE_WORDS):
                        g[(i + q) % (p.k + 1), (i + q) % L, (i + 1) % (p.k + 1), 3 * i + q:3 * i + q + 2] = U(w)
                    ggsws.append(g)
                ggsws = np.stack(ggsws)
                glwe = rng.integers(0, 2 ** 64, (GMAX, p.k + 1, p.N), dtype=U)
                for i, w in enumerate(EDGE_WORDS):
                    glwe[i % GMAX, i % (p.k + 1), 5 * i:5 * i + 3] = U(w)
                prec = beta * L
                ties = [((1 << (beta - 1)) << (64 - beta * l)) | (c << (62 - prec - (L - l)))
                        for l in range(1, L + 1) for c in (0, 1)]
                for g in (0, 1, 16):
                    glwe[g, (g + p.k) % (p.k + 1), 40:40 + len(ties)] = np.array(ties, U)
                self.host[t, (beta, L)] = (ggsws, glwe)
                self.dev[t, (beta, L)] = (dev_u64(eng, ggsws), dev_u64(eng, glwe))

    @lru_cache(maxsize=None)
    def prod(self, t, gadget, q, G):
        ggsws, glwe = self.host[t, gadget]
        return X.external_product(glwe[:G], ggsws[q], gadget[0])

    def item(self, t, gadget, spec, eng=None):
        """(ggsws, base_log, level, docs, B, D) of tenant t for spec (Q, G, D)."""
        if spec is None:
            return None
        Qn, G, D = spec
        eng = eng or self.engines[t]
        gg, gl = self.dev[t, gadget]
        words = eng.ggsw_words(*gadget)
        B = shape(self.p, G, D)
        docs = eng.pack_docs_glwe_queries(gl[:G].contiguous(), B, D, *gadget)
        return (gg.reshape(-1)[:Qn * words].contiguous(), gadget[0], gadget[1], docs, B, D)

    def own(self, t, item, csts):
        return u64(self.engines[t].linear_ggsws(*item, csts)).reshape(-1, self.W)

    def run(self, gadget, specs, group=None, order=None, check_ref=True):
        """The group call on specs (one (Q, G, D) or None per tenant, tenant
        order `order`) into a sentinel buffer of M + 16 rows. Checks every
        tenant's rows against its own call (and the restatement), the padding
        and trailing rows against the sentinel. Returns {tenant: rows}."""
        order = list(range(len(specs))) if order is None else order
        items = [self.item(t, gadget, s) for t, s in zip(order, specs)]
        csts = [None if s is None else CSTS[t:t + s[0]] if t + s[0] <= len(CSTS) else CSTS[:s[0]]
                for t, s in zip(order, specs)]
        counts = [0 if it is None else (it[0].numel() // self.engines[0].ggsw_words(*gadget)) * it[4] for it in items]
        M, starts = group_rows(counts)
        dev = self.engines[0].device
        buf = torch.full((M + 16, self.W), SENT, dtype=torch.int64, device=dev)
        owns = [None if it is None else self.own(t, it, cs) for t, it, cs in zip(order, items, csts)]
        out = (group or self.group).linear_ggsws(items, csts, out=buf)   # last: tenant 0's bucket names this launch
        assert out.data_ptr() == buf.data_ptr()
        torch.cuda.synchronize()
        got = u64(buf).reshape(M + 16, self.W)
        real = np.zeros(M + 16, bool)
        res = {}
        for t, s, it, cs, n, st, own in zip(order, specs, items, csts, counts, starts, owns):
            if it is None:
                continue
            Qn, G, D = s
            B = it[4]
            real[st:st + n] = True
            rows = got[st:st + n]
            np.testing.assert_array_equal(rows, own, err_msg=f"tenant {t} against its own call")
            if check_ref:
                for q in range(Qn):
                    want = X.extract_slots(self.prod(t, gadget, q, G), B, D, (cs[q] << (64 - self.p.msg_bits)) % 2 ** 64)
                    np.testing.assert_array_equal(rows[q * B:(q + 1) * B], want,
                                                  err_msg=f"tenant {t} query {q} against the restatement")
            res[t] = rows.copy()
        assert (got[~real] == np.array(SENT, np.int64).view(U)).all(), "a padding or trailing row was written"
        return res, counts, starts


@pytest.fixture(scope="module")
def ten(need_gpu):
    return Tenants()


# One launch each. A: Q_t in {11, 1, 6} = 33, 3 and 18 rows (RT = 2, the
# one-tile tenant padded to a tile pair), G in {2, 17, 1}, D in {256, 5, 16},
# Q_t B_t = 22, 833, 6 (padding rows). B: all Q_t = 1 (RT = 1), D = 1.
# C, D, E: a tenant sitting out first, in the middle, last.
MIXES = {
    "A": ((4, 3), [(11, 2, 256), (1, 17, 5), (6, 1, 16)]),
    "B": ((7, 7), [(1, 17, 1), (1, 2, 5), (1, 1, 16)]),
    "C": ((7, 7), [None, (6, 2, 256), (11, 1, 1)]),
    "D": ((4, 3), [(1, 1, 16), None, (2, 17, 5)]),
    "E": ((7, 7), [(6, 2, 5), (1, 1, 256), None]),
}


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_group_leveled_step_word_for_word(ten, mix):
    gadget, specs = MIXES[mix]
    e0 = ten.engines[0]
    res, counts, starts = ten.run(gadget, specs)
    rt = 2 if any(s and 3 * s[0] > 16 for s in specs) else 1
    assert e0.kernel_name("linear_ggsws") == f"k_extprod_queries_mfma_grp<{rt}>"
    assert any(n % 4 for n in counts), "the mix has padding rows"
    live = sorted(res)
    a, b = res[live[0]], res[live[1]]
    n = min(len(a), len(b))
    assert (a[:n] != b[:n]).any(), "two tenants' rows differ"


def test_group_of_one_tenant(ten):
    grp = EngineGroup([ten.engines[1]])
    item = ten.item(1, (7, 7), (6, 2, 16))
    got = u64(grp.linear_ggsws([item], [CSTS[:6]])).reshape(-1, ten.W)
    M, _ = group_rows([6 * item[4]])
    assert len(got) == M
    np.testing.assert_array_equal(got[:6 * item[4]], ten.own(1, item, CSTS[:6]))
    # every tenant sitting out is FHE_OK and launches nothing
    assert grp.linear_ggsws([None], [None]).numel() == 0
    grp.close()


def test_group_canaries_and_inputs_only_read(ten):
    """Mix A into a sentinel buffer (Tenants.run asserts the padding rows and
    the 16 rows past M); the GGSWs and the document operands are unchanged."""
    gadget, specs = MIXES["A"]
    items = [ten.item(t, gadget, s) for t, s in enumerate(specs)]
    before = [(it[0].clone(), it[3].clone()) for it in items]
    counts = [s[0] * it[4] for s, it in zip(specs, items)]
    M, starts = group_rows(counts)
    assert M > sum(counts)
    buf = torch.full((M + 16, ten.W), SENT, dtype=torch.int64, device=ten.engines[0].device)
    ten.group.linear_ggsws(items, [CSTS[:s[0]] for s in specs], out=buf)
    torch.cuda.synchronize()
    for (g0, d0), it in zip(before, items):
        assert torch.equal(g0, it[0]) and torch.equal(d0, it[3])
    real = np.zeros(M + 16, bool)
    for n, st in zip(counts, starts):
        real[st:st + n] = True
    assert (buf.cpu().numpy()[~real] == SENT).all() and (buf.cpu().numpy()[real, -1] != SENT).all()


def test_group_unsplit_path(ten):
    """Three tenants with Q = 1, D = 256, B = G = 48: 3 x 96 = 288 tiles, so the
    split rule max(1, min(KB / 4, 512 // tiles)) gives S = 1 (plain stores, no
    memset), while each tenant alone (96 tiles) runs S = 5 with atomics. The
    words are equal."""
    p, gadget = TOY, (4, 3)
    G = B = 48
    KB = (p.k + 1) * p.N * gadget[1] // 64
    tiles = G * (p.N // 16) // 8
    assert tiles == 96 and max(1, min(KB // 4, 512 // (3 * tiles))) == 1 and max(1, min(KB // 4, 512 // tiles)) == 5
    items, csts = [], []
    for t, eng in enumerate(ten.engines):
        rng = np.random.default_rng(4800 + t)
        gl = dev_u64(eng, rng.integers(0, 2 ** 64, (G, p.k + 1, p.N), dtype=U))
        docs = eng.pack_docs_glwe_queries(gl, B, 256, *gadget)
        gg = ten.dev[t, gadget][0].reshape(-1)[:eng.ggsw_words(*gadget)].contiguous()
        items.append((gg, gadget[0], gadget[1], docs, B, 256))
        csts.append([CSTS[t]])
    got = u64(ten.group.linear_ggsws(items, csts)).reshape(-1, ten.W)
    M, starts = group_rows([B] * 3)
    assert len(got) == M
    for t in range(3):
        np.testing.assert_array_equal(got[starts[t]:starts[t] + B], ten.own(t, items[t], csts[t]), err_msg=f"tenant {t}")


def test_group_rows_do_not_depend_on_company_or_order(ten):
    gadget = (7, 7)
    specs = [(6, 2, 5), (1, 17, 16), (11, 1, 256)]
    together, _, _ = ten.run(gadget, specs, check_ref=False)
    alone, _, _ = ten.run(gadget, [None, specs[1], None], check_ref=False)
    np.testing.assert_array_equal(alone[1], together[1])
    order = [2, 0, 1]
    grp = EngineGroup([ten.engines[t] for t in order])
    perm, _, _ = ten.run(gadget, [specs[t] for t in order], group=grp, order=order, check_ref=False)
    for t in range(3):
        np.testing.assert_array_equal(perm[t], together[t], err_msg=f"tenant {t} in another order")
    grp.close()


def test_group_profile_goes_to_tenant_0(ten):
    """Tenant 0 sits out; its "linear_ggsws" bucket still takes the one bracket."""
    gadget, specs = MIXES["C"]
    e0 = ten.engines[0]
    e0.profile(True)
    e0.profile_read("linear_ggsws")
    _, counts, _ = ten.run(gadget, specs, check_ref=False)
    e0.profile(False)
    assert e0.kernel_name("linear_ggsws") == "k_extprod_queries_mfma_grp<2>"
    r = e0.profile_read("linear_ggsws")
    assert r["launches"] == 1 and r["items"] == sum(counts) and r["total_ms"] > 0


def test_group_rejections(ten):
    L = _lib.lib()
    grp = ten.group
    gadget = (4, 3)
    specs = [(1, 1, 16), (2, 1, 5), (1, 2, 16)]
    items = [ten.item(t, gadget, s) for t, s in enumerate(specs)]
    ks = [np.array(CSTS[:s[0]], np.int64) for s in specs]
    ptrs = (C.c_void_p * 3)(*[k.ctypes.data for k in ks])
    out = torch.empty((16, ten.W), dtype=torch.int64, device=ten.engines[0].device)
    st = C.c_void_p(torch.cuda.current_stream(ten.engines[0].device).cuda_stream)

    def linear(mutate):
        arr, _ = grp._ggsw_items(items)
        mutate(arr)
        rc = L.fhe_linear_ggsws_group_batch(grp._grp, arr, 3, ptrs, C.c_void_p(out.data_ptr()), st)
        return rc, L.fhe_last_error(None)

    def level(arr):
        arr[1].level = 2
    def size(arr):
        arr[2].struct_size = 8
    def dim(arr):
        arr[0].D = TOY.N + 1
    def null(arr):
        arr[1].d_docs = None
    def reserved(arr):
        arr[2].reserved = 1
    for mutate, who, what in ((level, b"tenant 1", b"level"), (size, b"tenant 2", b"struct_size"),
                              (dim, b"tenant 0", b"D > N"), (null, b"tenant 1", b"null"),
                              (reserved, b"tenant 2", b"reserved")):
        rc, msg = linear(mutate)
        assert rc == E_ARG and who in msg and what in msg, (mutate.__name__, rc, msg)
    assert L.fhe_linear_ggsws_group_batch(grp._grp, grp._ggsw_items(items)[0], 2, ptrs, None, st) == E_ARG
    # the search entry: levels_bit, then a participating tenant without a packing key
    search = [it + (0, [0] * s[0], 9 if t == 2 else 0) for t, (it, s) in enumerate(zip(items, specs))]
    with pytest.raises(_lib.FheError, match="FHE_E_ARG.*tenant 2.*levels_bit"):
        grp.search_ggsws(search)
    search = [it + (0, [0] * s[0], 0) for it, s in zip(items, specs)]
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*tenant 0"):
        grp.search_ggsws(search)
    assert grp.search_ggsws([None, None, None]) == [None, None, None]


# -------------------------------------------------------- through PrivateHub --
def hub_case(hub, tenants):
    """tenants: {name: (client, cq, oq, n_e, qs, docs, ts)}. Runs the hub and
    every tenant's own server; checks replies word for word, decrypted values
    against the clear restatement."""
    requests, want = {}, {}
    for name, (client, cq, oq, n_e, qs, docs, ts) in tenants.items():
        B = hub.load(name, client.encrypt_docs(docs))
        assert B == len(docs)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_e, q, docs) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        below = np.stack([np.zeros(B, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                          for q, t in enumerate(ts)])
        requests[name] = (client.encrypt_queries(qs), ts)
        want[name] = (ref, below)
    got = hub.search_many(requests)
    assert list(got) == list(requests)
    first = next(iter(hub.tenants.values()))["server"].engine
    assert first.kernel_name("linear_ggsws").startswith("k_extprod_queries_mfma_grp<")   # the hub ran the group form
    for name, (client, *_rest) in tenants.items():
        rec = hub.tenants[name]
        own = rec["server"].search_many(requests[name][0], rec["docs"], rec["B"], requests[name][1])
        assert len(got[name]) == len(own) == 1
        np.testing.assert_array_equal(got[name][0], own[0], err_msg=f"{name}: reply words against its own server")
        for replies in (got[name], own):
            acc, below = client.decrypt_replies(replies)
            np.testing.assert_array_equal(acc.cpu().numpy(), want[name][0], err_msg=name)
            np.testing.assert_array_equal(below.cpu().numpy(), want[name][1], err_msg=name)
    return want, requests


def test_private_hub_toy_end_to_end(need_gpu):
    """The 5-feature, 2-bit model of tests/test_gpu_group.py (P0 = 8), the
    gadget planned by plan_gadget: three tenants with their own keys, (Q, B) =
    (3, 130), (1, 1), (2, 17); thresholds None, a fixed value and a median."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.model import QuantParams
    from fheicp.private import PrivateClient, PrivateHub
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    cq = CorpusQuant(qp, 2, 0.5)
    oq = Q.QuantizedLinearParams.from_json(qp.to_dict())
    shapes = {"alice": (3, 130), "bob": (1, 1), "carol": (2, 17)}
    made = {}
    for i, (name, (Qn, B)) in enumerate(shapes.items()):
        rng = np.random.default_rng(77 + i)
        qs = rng.uniform(-1.2, 0.7, (Qn, 5)).astype(np.float32)
        docs = rng.uniform(-1.2, 0.7, (B, 5)).astype(np.float32)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 2, q, docs) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        med = float(np.median(scores[Qn // 2]))
        ts = {"alice": [None, med, 0.5], "bob": [0.5], "carol": [None, med]}[name]
        if name != "bob":                                   # the clear restatement: bits on both sides
            assert 0 < int((scores[Qn // 2] < med).sum()) < B
        made[name] = (qs, docs, ts)
    hub, tenants = PrivateHub(0), {}
    for i, name in enumerate(shapes):
        c = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=99 + i, device=0, noise_seed=6 + i)
        assert c.P0 == 8
        client = PrivateClient(c, count=TOY.N, pack_seed=17 + i, enc_seed=12 + i)
        server = hub.add_tenant(name, client.eval_keys(), cq, c.P0, scheme=c.scheme)
        assert (server.base_log, server.level) == client.gadget
        tenants[name] = (client, cq, oq, 2) + made[name]
    with pytest.raises(ValueError, match="'dave'.*P0"):
        hub.add_tenant("dave", {}, cq, 12, scheme=TOY)
    with pytest.raises(ValueError, match="'alice' has no documents"):
        hub.search_many({"alice": ([], None)})
    want, requests = hub_case(hub, tenants)
    assert 0 < want["alice"][1][1].sum() < 130 and 0 < want["carol"][1][1].sum() < 17
    with pytest.raises(ValueError, match="unknown tenant 'erin'"):
        hub.search_many({"erin": ([], None)})
    # one tenant alone goes through its own server
    only = hub.search_many({"carol": requests["carol"]})
    acc, below = tenants["carol"][0].decrypt_replies(only["carol"])
    np.testing.assert_array_equal(acc.cpu().numpy(), want["carol"][0])
    np.testing.assert_array_equal(below.cpu().numpy(), want["carol"][1])
    hub.close()


def test_private_hub_real_parameters_p21(need_gpu):
    """The 16-dim, n_bits 6 model (P0 = 21, gadget (7, 6)), two tenants with
    different keys, (Q, B) = (1, 5) and (2, 3)."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.private import PrivateClient, PrivateHub
    Xt, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(Xt, y, 6)
    oq = Q.fit_quantized_linear(Xt, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    hub, tenants = PrivateHub(0), {}
    for i, (name, (Qn, B)) in enumerate({"alice": (1, 5), "bob": (2, 3)}.items()):
        c = EncryptedCorpus(cq).compile(key_seed=5 + i, device=0, noise_seed=6 + i)
        assert c.P0 == 21
        client = PrivateClient(c, count=256, pack_seed=4 + i, enc_seed=12 + i)
        assert client.gadget == (7, 6)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, scheme=c.scheme)
        qs, docs = [], None
        for j in range(Qn):
            q, d = Q.make_corpus(16, B, seed=40 + 10 * i + j)
            qs.append(q)
            docs = d if docs is None else docs
        ts = [0.5] if Qn == 1 else [None, 0.5]
        tenants[name] = (client, cq, oq, 6, np.stack(qs), docs, ts)
    hub_case(hub, tenants)
    hub.close()
