"""CPU: the bridge key switch of a stored-ciphertext key rotation (DESIGN.md
§8.12) as far as it goes without a device: the numpy restatement
(tests/bridge_ref.py) round-trips messages from one key to another with the
model's noise, the gadget plan in C and in Python, key sizes, the argument
refusals on a host-only context in their stated order, and CorpusServer's
rekey / append / load bookkeeping against a stub engine."""
import ctypes as C
import math

import numpy as np
import pytest

import bridge_ref as BR
from fheicp import _lib
from fheicp.params import TOY, bridge_plan, bridge_var, pack_plan, pack_sigmas, params_for_bits

U = np.uint64
IN_VAR = (2.0 ** -33) ** 2


def host_ctx(p):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(_lib.params_struct(p.as_dict())), -1, C.byref(h)) == 0
    return L, h


def test_restatement_round_trip_on_toy():
    """4096 TOY encryptions of known messages under a random s_old, bridged
    with a numpy-made key, read under s_new: every message comes back and the
    sigma of the error the bridge adds (new phase minus old phase) is the
    model's to within 10% (the sampling error of sigma from 4096 values is
    1.1%)."""
    p = TOY
    big = p.k * p.N
    rng = np.random.default_rng(31)
    s_old, s_new = rng.integers(0, 2, big, dtype=U), rng.integers(0, 2, big, dtype=U)
    beta, lv = bridge_plan(p, 0.0)
    bk = BR.make_bridge_key(rng, s_old, s_new, beta, lv, p.glwe_noise_bits)
    assert bk.shape == (big, lv, big + 1)
    # the key rows decrypt to their messages with TUniform noise
    ph = BR.lwe_phase(bk.reshape(-1, big + 1), s_new).reshape(big, lv)
    with np.errstate(over="ignore"):
        for l in range(lv):
            ph[:, l] -= s_old << U(64 - beta * (l + 1))
    assert np.abs(ph.astype(np.int64)).max() <= 1 << p.glwe_noise_bits
    P = p.msg_bits
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), 4096)
    msgs[:4] = (-(1 << (P - 1)), (1 << (P - 1)) - 1, 0, -1)
    ct = BR.encrypt_lwe(rng, msgs, s_old, P, p.glwe_noise_bits)
    np.testing.assert_array_equal(BR.decode(BR.lwe_phase(ct, s_old), P), msgs)
    phase = BR.bridge_phase_ref(ct, bk, s_new, beta, lv)
    # the shortcut is the full restatement's phase
    full = BR.bridge_ref(ct[:64], bk, beta, lv)
    assert full.shape == (64, big + 1)
    np.testing.assert_array_equal(BR.lwe_phase(full, s_new), phase[:64])
    sub = BR.bridge_ref(ct[:64], bk, beta, lv, cols=[0, 7, big - 1, big])
    np.testing.assert_array_equal(sub, full[:, [0, 7, big - 1, big]])
    np.testing.assert_array_equal(BR.decode(phase, P), msgs)
    err = (phase - BR.lwe_phase(ct, s_old)).astype(np.int64)
    sigma = math.sqrt(BR.bridge_var(p, beta, lv))
    assert BR.bridge_var(p, beta, lv) == bridge_var(p, beta, lv)
    print(f"bridge sigma / model = {err.std() / sigma:.4f}")
    assert 0.9 * sigma <= err.std() <= 1.1 * sigma
    assert np.abs(err).max() <= 6 * sigma


# the issue's table at in_var = (2^-33)^2, count 1024: P -> bridge gadget, its
# margin, the reply packing's gadget and margin (sigmas)
TABLE = {8: ((7, 3), 443, (7, 3), 313), 16: ((7, 4), 222, (7, 4), 157), 21: ((7, 5), 812, (7, 5), 377),
         24: ((7, 5), 101, (7, 5), 47), 26: ((7, 5), 25.4, (7, 5), 11.8), 27: ((7, 5), 12.7, (5, 8), 11.2)}


def test_bridge_plan_matches_library_and_keeps_the_packing_bar():
    L = _lib.lib()
    for p, in_var in [(TOY, 0.0), (TOY, IN_VAR)] + [(params_for_bits(P), IN_VAR) for P in range(4, 28)]:
        cp = _lib.params_struct(p.as_dict())
        b, lv = C.c_int32(), C.c_int32()
        assert L.fhe_bridge_plan(C.byref(cp), in_var, C.byref(b), C.byref(lv)) == 0
        got = (b.value, lv.value)
        assert got == bridge_plan(p, in_var) == pack_plan(p, 1, in_var)[:2], p.msg_bits
        if p is TOY:
            continue
        P = p.msg_bits
        margin = 2.0 ** (63 - P) / math.sqrt(in_var * 2.0 ** 128 + BR.bridge_var(p, *got))
        assert margin >= 9.2, P
        # the packing key that follows, planned with the bridge's variance added
        iv2 = in_var + BR.bridge_var(p, *got) / 2.0 ** 128
        pb, pl, _ = pack_plan(p, 1024, iv2)
        pm = pack_sigmas(p, 1024, iv2, pb, pl, 63 - P)
        assert pm >= 9.2, (P, pm)
        if P in TABLE:
            g, m, pg, pmar = TABLE[P]
            assert got == g and (pb, pl) == pg, P
            assert abs(margin - m) <= 0.006 * m + 0.05 and abs(pm - pmar) <= 0.006 * pmar + 0.05, (P, margin, pm)
    assert pack_plan(params_for_bits(27), 1024, IN_VAR)[:2] == (6, 6)      # "was (6,6)" without the bridge
    assert L.fhe_bridge_plan(C.byref(cp), -1.0, None, None) == -1
    assert L.fhe_bridge_plan(C.byref(cp), float("nan"), None, None) == -1
    assert L.fhe_bridge_plan(C.byref(cp), 0.0, None, None) == 0
    assert L.fhe_bridge_plan(None, 0.0, None, None) == -1


def test_bridge_key_words():
    L = _lib.lib()
    for p in (TOY, params_for_bits(16)):
        P = _lib.params_struct(p.as_dict())
        kN = p.k * p.N
        for beta, lv in ((4, 3), (7, 6), (6, 4), (1, 1), (6, 8)):
            assert L.fhe_bridge_key_words(C.byref(P), beta, lv) == kN * lv * (kN + 1)
        for beta, lv in ((0, 3), (8, 3), (4, 0), (4, 9), (7, 8)):
            assert L.fhe_bridge_key_words(C.byref(P), beta, lv) == 0
    assert L.fhe_bridge_key_words(None, 4, 3) == 0


def test_bridge_refusals_on_host_context_in_order():
    """Argument errors are FHE_E_ARG (-1) even on a host-only context and come
    before the device check (-2): bad gadget, then null pointers, then a key
    word other than 0 or 1; B_old outside [0, B] for the search entry."""
    L, h = host_ctx(TOY)
    big = TOY.k * TOY.N
    key = (C.c_uint32 * 8)(*range(8))
    buf = (C.c_uint64 * 64)()
    hv = (C.c_int64 * 4)()
    s_ok = (C.c_uint64 * big)(*([1, 0] * (big // 2)))
    s_bad = (C.c_uint64 * big)(*([1, 0] * (big // 2)))
    s_bad[big - 1] = 2
    err = lambda: L.fhe_last_error(h)  # noqa: E731
    for beta, lv in ((0, 3), (8, 3), (4, 0), (4, 9), (7, 8)):
        # the gadget is refused first: with a null key, a null secret and a bad word behind it
        assert L.fhe_keygen_bridge_key(h, None, beta, lv, 1, None) == -1 and b"bridge gadget" in err()
        assert L.fhe_keygen_bridge_key_key(h, s_bad, beta, lv, None, None) == -1 and b"bridge gadget" in err()
        assert L.fhe_import_bridge_key(h, beta, lv, None) == -1 and b"bridge gadget" in err()
    for beta, lv in ((4, 3), (7, 7), (6, 8)):
        assert L.fhe_keygen_bridge_key(h, None, beta, lv, 1, None) == -1 and b"null" in err()
        assert L.fhe_keygen_bridge_key_key(h, s_bad, beta, lv, None, None) == -1 and b"null" in err()
        assert L.fhe_keygen_bridge_key_key(h, None, beta, lv, key, None) == -1 and b"null" in err()
        assert L.fhe_keygen_bridge_key(h, s_bad, beta, lv, 1, None) == -1 and b"0 or 1" in err()
        assert L.fhe_keygen_bridge_key_key(h, s_bad, beta, lv, key, None) == -1 and b"0 or 1" in err()
        assert L.fhe_keygen_bridge_key(h, s_ok, beta, lv, 1, None) == -2 and b"host-only" in err()
        assert L.fhe_keygen_bridge_key_key(h, s_ok, beta, lv, key, None) == -2
        assert L.fhe_import_bridge_key(h, beta, lv, None) == -1 and b"null" in err()
        assert L.fhe_import_bridge_key(h, beta, lv, buf) == -2
    assert L.fhe_export_bridge_key(h, None) == -1
    assert L.fhe_export_bridge_key(h, buf) == -2
    assert L.fhe_bridge_batch(h, buf, -1, buf, None) == -1 and b"bridge" in err()
    assert L.fhe_bridge_batch(h, None, 4, buf, None) == -1
    assert L.fhe_bridge_batch(h, buf, 4, None, None) == -1
    assert L.fhe_bridge_batch(h, buf, 4, buf, None) == -2
    assert L.fhe_bridge_batch(h, None, 0, None, None) == -2           # nothing to refuse but the device
    assert L.fhe_bridge_batch(None, buf, 4, buf, None) == -1

    def sea(Q, B, D, B_old, W=buf, hT=hv, lb=0):
        return L.fhe_search_seeded_queries_bridged_batch(h, buf, buf, B, D, key, Q, W, 0, hT, lb, B_old, buf, buf, None)

    for Qn, B, D in ((0, 4, 16), (2, 0, 16), (2, 4, 0), (65536, 4, 16)):
        assert sea(Qn, B, D, 0) == -1 and b"seeded queries" in err()
    assert sea(2, 4, 16, 0, lb=9) == -1
    assert sea(2, 4, 16, 2, W=None) == -1 and b"null" in err()
    assert sea(2, 4, 16, 2, hT=None) == -1
    for B_old in (-1, 5, 2 ** 40):
        assert sea(2, 4, 16, B_old) == -1 and b"B_old" in err(), B_old
    for B_old in (0, 1, 4):
        assert sea(2, 4, 16, B_old) == -2 and b"host-only" in err(), B_old
    nm = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"bridge", nm, 64) == 0 and nm.value == b""
    L.fhe_ctx_destroy(h)


# ------------------------------------------------- CorpusServer bookkeeping --
class StubEngine:
    """Stands for fheicp.engine.Engine in CorpusServer: records what the
    server asks of it and keeps buffers as CPU tensors."""

    def __init__(self, scheme):
        self.params = scheme
        self.imported, self.searches = [], []

    def import_eval_keys(self, d):
        self.imported.append(d)

    def to_dev(self, a):
        import torch
        a = np.ascontiguousarray(a)
        return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy())

    def set_msg_bits(self, P):
        self.params = self.params.with_msg_bits(P)

    def search_seeded_queries(self, body, ids, mask_key, W, cst, Ts, levels_bit=0, b_old=0):
        import torch
        self.searches.append({"B": int(body.shape[0]), "b_old": int(b_old), "Q": len(Ts)})
        n1 = (self.params.k + 1) * self.params.N
        G = -(-(len(Ts) * int(body.shape[0])) // self.params.N)
        return torch.zeros((G, n1), dtype=torch.int64), torch.zeros((G, n1), dtype=torch.int64)


def fake_keys(gen: int, bridge_from=None):
    from fheicp.stored import key_fingerprint
    ksk = np.arange(8, dtype=U) + U(1000 * gen)
    d = {"bsk": np.zeros(4, U), "ksk": ksk, "pack_key": np.zeros(4, U), "pack_gadget": np.array([4, 3]),
         "pack_bit_levels": np.array([1 + gen]), "key_id": np.array([key_fingerprint(ksk)])}
    if bridge_from is not None:
        d.update(bridge_key=np.zeros(4, U), bridge_gadget=np.array([7, 3]), bridge_from=np.array([bridge_from]))
    return d


@pytest.fixture(scope="module")
def stub_server():
    from oracle import quant_ref as Q
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.stored import CorpusServer
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))

    class Server(CorpusServer):
        def _make_engine(self, device):
            return StubEngine(self.scheme)

    return lambda keys: Server(keys, cq, EncryptedCorpus(cq).P0, np.arange(8, dtype=np.uint32)), cq


def test_server_rekey_append_load_bookkeeping(stub_server):
    from fheicp.stored import key_fingerprint
    make, cq = stub_server
    k0 = fake_keys(0)
    id0, id1, id2, id3 = (key_fingerprint(fake_keys(g)["ksk"]) for g in range(4))
    assert len({id0, id1, id2, id3}) == 4 and all(len(i) == 16 and int(i, 16) >= 0 for i in (id0, id1))
    s = make(k0)
    assert (s.key_id, s.b_old, s.old_key_id) == (id0, 0, None)
    rng = np.random.default_rng(1)
    docs = lambda n: (rng.integers(0, 2 ** 64, (n, 16), dtype=U), rng.integers(0, 2 ** 64, n, dtype=U))  # noqa: E731
    q = np.zeros((2, 16), np.float32)
    # a rekey with nothing resident needs no bridge
    s.rekey(fake_keys(0))
    assert s.b_old == 0
    assert s.load(*docs(12)) == 12 and s.b_old == 0
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 12, "b_old": 0, "Q": 2}
    # documents resident: the new keys must bridge from THEIR generation
    with pytest.raises(ValueError, match="no bridge key"):
        s.rekey(fake_keys(1))
    with pytest.raises(ValueError, match="bridge key comes from"):
        s.rekey(fake_keys(1, bridge_from=id3))
    assert (s.key_id, s.b_old) == (id0, 0) and len(s.engine.imported) == 2     # refused before anything changed
    k1 = fake_keys(1, bridge_from=id0)
    s.rekey(k1)
    assert (s.key_id, s.b_old, s.old_key_id, s.bit_levels) == (id1, 12, id0, 2)
    assert s.engine.imported[-1] is k1
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 12, "b_old": 12, "Q": 2}
    assert s.append(*docs(5)) == 17 and s.b_old == 12
    s.search(q[0])
    assert s.engine.searches[-1] == {"B": 17, "b_old": 12, "Q": 1}
    assert s.append(*docs(3)) == 20 and s.b_old == 12
    with pytest.raises(ValueError, match="features"):
        s.append(rng.integers(0, 2 ** 64, (2, 15), dtype=U), np.zeros(2, U))
    # a second rotation: generation-0 documents are resident, so the bridge
    # must come from generation 0, and no newer generation may be resident
    with pytest.raises(ValueError, match=id0):
        s.rekey(fake_keys(2, bridge_from=id1))
    with pytest.raises(ValueError, match="two generations"):
        s.rekey(fake_keys(2, bridge_from=id0))
    assert (s.key_id, s.b_old, s.old_key_id) == (id1, 12, id0)
    body, ids = s.body[:12].numpy().view(U), s.ids[:12].numpy().view(U)
    assert s.load(body, ids) == 12 and (s.b_old, s.old_key_id) == (0, None)    # load resets
    # (the host reloads only the generation-0 documents and says so)
    s.b_old, s.old_key_id = 12, id0
    s.rekey(fake_keys(2, bridge_from=id0))
    assert (s.key_id, s.b_old, s.old_key_id) == (id2, 12, id0)
    s.append(*docs(4))
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 16, "b_old": 12, "Q": 2}
    # append on an empty server is a load
    s2 = make(k0)
    assert s2.append(*docs(3)) == 3 and s2.b_old == 0


def test_eval_keys_file_carries_the_bridge_entries(tmp_path, stub_server):
    """save_eval_keys / load_eval_keys (plain arrays, no pickles) keep
    bridge_key, bridge_gadget, bridge_from and key_id, and a server rekeys
    from the loaded dict."""
    from fheicp.query import load_eval_keys, save_eval_keys
    from fheicp.stored import key_fingerprint
    make, _ = stub_server
    id0 = key_fingerprint(fake_keys(0)["ksk"])
    k1 = fake_keys(1, bridge_from=id0)
    path = str(tmp_path / "eval.npz")
    save_eval_keys(path, k1)
    got = load_eval_keys(path)
    assert set(got) == set(k1)
    for name in ("bridge_key", "bridge_gadget", "ksk"):
        np.testing.assert_array_equal(got[name], k1[name])
    assert str(got["bridge_from"][0]) == id0 and str(got["key_id"][0]) == str(k1["key_id"][0])
    s = make(fake_keys(0))
    s.load(np.zeros((3, 16), U), np.arange(3, dtype=U))
    s.rekey(got)
    assert (s.b_old, s.old_key_id, s.key_id) == (3, id0, str(k1["key_id"][0]))


def test_rotated_client_ids_do_not_overlap():
    """CorpusClient's id bookkeeping without a device: a rotated client's
    default ids are consecutive runs of D after every id the old client
    handed out."""
    from fheicp.stored import CorpusClient

    class FakeCorpus:
        def encrypt_docs(self, docs, id0=None):
            B = len(docs)
            ids = (np.arange(B, dtype=U) * U(1000) + U(77) if id0 is None else np.asarray(id0, dtype=U).reshape(B))
            return np.zeros((B, docs.shape[1]), U), ids

    def client(next_id):
        c = CorpusClient.__new__(CorpusClient)
        c.corpus = FakeCorpus()
        c.next_id = next_id
        c._id_end = 0 if next_id is None else next_id
        return c

    old = client(None)
    D = 16
    _, ids_a = old.encrypt_docs(np.zeros((12, D)))
    _, ids_b = old.encrypt_docs(np.zeros((3, D)), id0=[5, 900000, 40])
    used_old = {int(i) + j for i in np.concatenate([ids_a, ids_b]) for j in range(D)}
    assert old.id_end == max(used_old) + 1 == 900000 + D
    new = client(old.id_end)
    _, ids_c = new.encrypt_docs(np.zeros((5, D)))
    _, ids_d = new.encrypt_docs(np.zeros((2, D)))
    used_new = [int(i) + j for i in np.concatenate([ids_c, ids_d]) for j in range(D)]
    assert len(set(used_new)) == 7 * D and not used_old & set(used_new)
    assert min(used_new) == old.id_end and new.id_end == max(used_new) + 1
