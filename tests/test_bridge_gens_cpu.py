"""CPU: key rotation with several old generations resident
as far as it goes without a device: the new entries' refusals on a host-only
context in their stated order (and the §8.12 entries unchanged on the same
context), CorpusServer's generation bookkeeping against a stub engine, the
evaluation-key file round trip of the multi-bridge entries, and a numpy
restatement of the segmented bridge (tests/bridge_ref.py per segment, three
key pairs) whose every segment decrypts under the new secret."""
import ctypes as C

import numpy as np
import pytest

import bridge_ref as BR
from fheicp import _lib
from fheicp.params import TOY, bridge_plan

U = np.uint64


def host_ctx(p):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(_lib.params_struct(p.as_dict())), -1, C.byref(h)) == 0
    return L, h


def i64s(*v):
    return (C.c_int64 * max(len(v), 1))(*v)


def i32s(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def test_bridge_slots_constant_matches_header():
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "fhe_icp.h").read_text()
    assert int(re.search(r"#define FHE_BRIDGE_SLOTS (\d+)", hdr).group(1)) == _lib.BRIDGE_SLOTS == 8


def test_slot_entries_refuse_on_host_context_in_order():
    """A slot outside [0, 8) is FHE_E_ARG before everything else; then the
    siblings' order: bad gadget, null pointers, a key word other than 0 or 1
    (all -1), then -2 "host-only"."""
    L, h = host_ctx(TOY)
    big = TOY.k * TOY.N
    key = (C.c_uint32 * 8)(*range(8))
    buf = (C.c_uint64 * 64)()
    s_ok = (C.c_uint64 * big)(*([1, 0] * (big // 2)))
    s_bad = (C.c_uint64 * big)(*([1, 0] * (big // 2)))
    s_bad[big - 1] = 2
    err = lambda: L.fhe_last_error(h)  # noqa: E731
    for slot in (-1, 8, 2 ** 20):
        # the slot is refused first: with a bad gadget, nulls and a bad word behind it
        assert L.fhe_keygen_bridge_key_slot(h, slot, None, 0, 3, 1, None) == -1 and b"bridge slot" in err()
        assert L.fhe_keygen_bridge_key_slot_key(h, slot, s_bad, 0, 3, None, None) == -1 and b"bridge slot" in err()
        assert L.fhe_keygen_bridge_key_slot_seeded(h, slot, s_bad, 0, 3, None, None, None) == -1
        assert b"bridge slot" in err()
        assert L.fhe_export_bridge_key_slot(h, slot, None) == -1 and b"bridge slot" in err()
        assert L.fhe_export_bridge_key_slot_seeded(h, slot, None, None) == -1 and b"bridge slot" in err()
        assert L.fhe_import_bridge_key_slot(h, slot, 0, 3, None) == -1 and b"bridge slot" in err()
        assert L.fhe_import_bridge_key_slot_seeded(h, slot, 0, 3, None, None) == -1 and b"bridge slot" in err()
        assert L.fhe_drop_bridge_key_slot(h, slot) == -1 and b"bridge slot" in err()
    for slot in (0, 3, 7):
        for beta, lv in ((0, 3), (8, 3), (4, 0), (4, 9), (7, 8)):
            assert L.fhe_keygen_bridge_key_slot(h, slot, None, beta, lv, 1, None) == -1 and b"bridge gadget" in err()
            assert L.fhe_keygen_bridge_key_slot_key(h, slot, s_bad, beta, lv, None, None) == -1
            assert b"bridge gadget" in err()
            assert L.fhe_keygen_bridge_key_slot_seeded(h, slot, s_bad, beta, lv, None, None, None) == -1
            assert b"seeded: bridge gadget" in err()
            assert L.fhe_import_bridge_key_slot(h, slot, beta, lv, None) == -1 and b"bridge gadget" in err()
            assert L.fhe_import_bridge_key_slot_seeded(h, slot, beta, lv, None, None) == -1
            assert b"seeded: bridge gadget" in err()
        for beta, lv in ((4, 3), (6, 8)):
            assert L.fhe_keygen_bridge_key_slot(h, slot, None, beta, lv, 1, None) == -1 and b"null" in err()
            assert L.fhe_keygen_bridge_key_slot_key(h, slot, s_bad, beta, lv, None, None) == -1 and b"null" in err()
            assert L.fhe_keygen_bridge_key_slot_key(h, slot, None, beta, lv, key, None) == -1 and b"null" in err()
            assert L.fhe_keygen_bridge_key_slot(h, slot, s_bad, beta, lv, 1, None) == -1 and b"0 or 1" in err()
            assert L.fhe_keygen_bridge_key_slot_key(h, slot, s_bad, beta, lv, key, None) == -1 and b"0 or 1" in err()
            assert L.fhe_keygen_bridge_key_slot_seeded(h, slot, s_ok, beta, lv, key, None, None) == -1
            assert b"seeded: null" in err()
            assert L.fhe_keygen_bridge_key_slot_seeded(h, slot, s_bad, beta, lv, key, key, None) == -1
            assert b"0 or 1" in err()
            assert L.fhe_keygen_bridge_key_slot(h, slot, s_ok, beta, lv, 1, None) == -2 and b"host-only" in err()
            assert L.fhe_keygen_bridge_key_slot_key(h, slot, s_ok, beta, lv, key, None) == -2
            assert L.fhe_keygen_bridge_key_slot_seeded(h, slot, s_ok, beta, lv, key, key, None) == -2
            assert L.fhe_import_bridge_key_slot(h, slot, beta, lv, None) == -1 and b"null" in err()
            assert L.fhe_import_bridge_key_slot(h, slot, beta, lv, buf) == -2 and b"host-only" in err()
            assert L.fhe_import_bridge_key_slot_seeded(h, slot, beta, lv, key, None) == -1 and b"null" in err()
            assert L.fhe_import_bridge_key_slot_seeded(h, slot, beta, lv, key, buf) == -2
        assert L.fhe_export_bridge_key_slot(h, slot, None) == -1 and b"null" in err()
        assert L.fhe_export_bridge_key_slot(h, slot, buf) == -2 and b"host-only" in err()
        assert L.fhe_export_bridge_key_slot_seeded(h, slot, key, None) == -1 and b"null" in err()
        assert L.fhe_export_bridge_key_slot_seeded(h, slot, key, buf) == -2
        assert L.fhe_drop_bridge_key_slot(h, slot) == -2 and b"host-only" in err()
    assert L.fhe_drop_bridge_key_slot(None, 0) == -1
    assert L.fhe_export_bridge_key_slot(None, 0, buf) == -1
    L.fhe_ctx_destroy(h)


def test_generation_entries_refuse_on_host_context_in_order():
    """Bad G, null tables, ends that decrease or exceed B, a slot out of range
    or named twice are -1 with the stated texts; then -2 "host-only". The
    §8.12 entries behave on the same context as they did."""
    L, h = host_ctx(TOY)
    key = (C.c_uint32 * 8)(*range(8))
    buf = (C.c_uint64 * 64)()
    hv = (C.c_int64 * 4)()
    err = lambda: L.fhe_last_error(h)  # noqa: E731

    def gens(Q, B, G, ends, slots, ct=buf):
        return L.fhe_bridge_gens_batch(h, ct, Q, B, G, ends, slots, None)

    def sea(Q, B, D, G, ends, slots, W=buf, hT=hv, lb=0):
        return L.fhe_search_seeded_queries_gens_batch(h, buf, buf, B, D, key, Q, W, 0, hT, lb, G, ends, slots, buf,
                                                      buf, None)

    for Qn, B in ((0, 4), (2, 0), (2 ** 31, 4), (2 ** 16, 2 ** 16)):
        assert gens(Qn, B, 0, None, None) == -1 and b"bridge generations" in err()
    for call in (lambda *a: gens(2, 8, *a), lambda *a: sea(2, 8, 16, *a)):
        for G in (-1, 9):
            assert call(G, i64s(1), i32s(0)) == -1 and b"G outside [0, 8]" in err()
        assert call(2, None, i32s(0, 1)) == -1 and b"null bridge generations tables" in err()
        assert call(2, i64s(1, 2), None) == -1 and b"null bridge generations tables" in err()
        for ends in ((3, 2), (-1, 2), (2, 9), (9, 9)):
            assert call(2, i64s(*ends), i32s(0, 1)) == -1 and b"ends must not decrease" in err(), ends
        for slots in ((0, 8), (-1, 0)):
            assert call(2, i64s(2, 4), i32s(*slots)) == -1 and b"bridge slot" in err()
        assert call(2, i64s(2, 4), i32s(3, 3)) == -1 and b"slot 3 named twice" in err()
        assert call(3, i64s(0, 0, 0), i32s(1, 2, 1)) == -1 and b"named twice" in err()
        # nothing left to refuse but the device
        assert call(0, None, None) == -2 and b"host-only" in err()
        assert call(2, i64s(2, 4), i32s(0, 1)) == -2 and b"host-only" in err()
        assert call(8, i64s(1, 2, 3, 4, 5, 6, 7, 8), i32s(7, 6, 5, 4, 3, 2, 1, 0)) == -2
        assert call(3, i64s(0, 0, 8), i32s(2, 0, 1)) == -2
    assert gens(2, 8, 1, i64s(2), i32s(0), ct=None) == -1 and b"null bridge buffers" in err()
    # the search entry's own checks come before the row map's
    for Qn, B, D in ((0, 4, 16), (2, 0, 16), (2, 4, 0), (65536, 4, 16)):
        assert sea(Qn, B, D, 9, None, None) == -1 and b"seeded queries" in err()
    assert sea(2, 4, 16, 9, None, None, lb=9) == -1 and b"levels_bit" in err()
    assert sea(2, 4, 16, 9, None, None, W=None) == -1 and b"null search" in err()
    assert sea(2, 4, 16, 9, None, None) == -1 and b"G outside" in err()
    assert L.fhe_bridge_gens_batch(None, buf, 1, 1, 0, None, None, None) == -1
    # the old entries on the same context, as tests/test_bridge_cpu.py pins them
    assert L.fhe_export_bridge_key(h, None) == -1 and L.fhe_export_bridge_key(h, buf) == -2
    assert L.fhe_import_bridge_key(h, 4, 3, None) == -1 and L.fhe_import_bridge_key(h, 4, 3, buf) == -2
    assert L.fhe_bridge_batch(h, buf, 4, buf, None) == -2 and L.fhe_bridge_batch(h, buf, -1, buf, None) == -1
    assert L.fhe_bridge_rows_batch(h, buf, 2, 4, 5, None) == -1 and b"B_old" in err()
    assert L.fhe_bridge_rows_batch(h, buf, 2, 4, 2, None) == -2
    assert L.fhe_search_seeded_queries_bridged_batch(h, buf, buf, 4, 16, key, 2, buf, 0, hv, 0, 5, buf, buf,
                                                     None) == -1 and b"B_old" in err()
    assert L.fhe_search_seeded_queries_bridged_batch(h, buf, buf, 4, 16, key, 2, buf, 0, hv, 0, 2, buf, buf,
                                                     None) == -2
    L.fhe_ctx_destroy(h)


# ------------------------------------------------- CorpusServer bookkeeping --
class StubEngine:
    """Stands for fheicp.engine.Engine in CorpusServer: records what the
    server asks of it, keeps buffers as CPU tensors and the bridge slots as a
    dict slot -> the imported row."""

    def __init__(self, scheme):
        self.params = scheme
        self.imported, self.searches, self.slots = [], [], {}

    def import_eval_keys(self, d):
        self.imported.append(d)
        if "bridge_key" in d:
            self.slots[0] = np.asarray(d["bridge_key"])
        if "bridge_keys" in d:
            rows = np.asarray(d["bridge_keys"])
            for g, row in enumerate(rows):
                self.slots[g] = row
            for s in [s for s in self.slots if s >= len(rows)]:
                del self.slots[s]

    def import_bridge_key(self, b, L, key, slot=0):
        self.slots[int(slot)] = np.asarray(key)

    def drop_bridge_key(self, slot):
        self.slots.pop(int(slot), None)

    def bridge_slots(self):
        return sorted(self.slots)

    def to_dev(self, a):
        import torch
        a = np.ascontiguousarray(a)
        return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy())

    def set_msg_bits(self, P):
        self.params = self.params.with_msg_bits(P)

    def _reply(self, body, Ts):
        import torch
        n1 = (self.params.k + 1) * self.params.N
        G = -(-(len(Ts) * int(body.shape[0])) // self.params.N)
        return torch.zeros((G, n1), dtype=torch.int64), torch.zeros((G, n1), dtype=torch.int64)

    def search_seeded_queries(self, body, ids, mask_key, W, cst, Ts, levels_bit=0, b_old=0):
        self.searches.append({"B": int(body.shape[0]), "b_old": int(b_old), "Q": len(Ts)})
        return self._reply(body, Ts)

    def search_seeded_queries_gens(self, body, ids, mask_key, W, cst, Ts, levels_bit=0, gen_ends=(), gen_slots=()):
        self.searches.append({"B": int(body.shape[0]), "ends": list(gen_ends), "slots": list(gen_slots),
                              "Q": len(Ts)})
        return self._reply(body, Ts)


def fake_keys(gen: int, bridge_from=None):
    """Evaluation keys of generation `gen`; bridge_from: a fingerprint (the
    single form) or a list of them (the multi form, row g = 100 + the source
    generation's position)."""
    from fheicp.stored import key_fingerprint
    ksk = np.arange(8, dtype=U) + U(1000 * gen)
    d = {"bsk": np.zeros(4, U), "ksk": ksk, "pack_key": np.zeros(4, U), "pack_gadget": np.array([4, 3]),
         "pack_bit_levels": np.array([1 + gen]), "key_id": np.array([key_fingerprint(ksk)])}
    if isinstance(bridge_from, list):
        d.update(bridge_keys=np.arange(len(bridge_from), dtype=U).reshape(-1, 1) + np.full((1, 4), 100, U),
                 bridge_gadget=np.array([7, 3]), bridge_from=np.array(bridge_from))
    elif bridge_from is not None:
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

    return lambda keys: Server(keys, cq, EncryptedCorpus(cq).P0, np.arange(8, dtype=np.uint32))


def test_server_generation_bookkeeping(stub_server):
    from fheicp.stored import key_fingerprint
    id0, id1, id2, id3 = (key_fingerprint(fake_keys(g)["ksk"]) for g in range(4))
    s = stub_server(fake_keys(0))
    rng = np.random.default_rng(1)
    docs = lambda n: (rng.integers(0, 2 ** 64, (n, 16), dtype=U), rng.integers(0, 2 ** 64, n, dtype=U))  # noqa: E731
    q = np.zeros((2, 16), np.float32)
    assert s.generations == [] and s.old_generations == []
    assert s.load(*docs(12)) == 12 and s.generations == [(id0, 12)]
    s.rekey(fake_keys(1, bridge_from=id0))
    assert s.append(*docs(5)) == 17
    assert s.old_generations == [(id0, 12)] and s.generations == [(id0, 12), (id1, 17)]
    # one old generation: the single bridge, exactly as before
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 17, "b_old": 12, "Q": 2}
    # a dict missing generation 1's bridge raises, naming it, and changes nothing
    n_imp = len(s.engine.imported)
    with pytest.raises(ValueError, match=id1):
        s.rekey(fake_keys(2, bridge_from=[id0]))
    with pytest.raises(ValueError, match=id0):
        s.rekey(fake_keys(2, bridge_from=[id1, id3]))
    assert len(s.engine.imported) == n_imp and (s.key_id, s.b_old, s.old_key_id, s.bit_levels) == (id1, 12, id0, 2)
    assert s.generations == [(id0, 12), (id1, 17)]
    # the single form cannot carry two generations either (the rule of §8.12)
    with pytest.raises(ValueError, match="two generations"):
        s.rekey(fake_keys(2, bridge_from=id0))
    # two bridges, with one for a generation that is not resident in between
    k2 = fake_keys(2, bridge_from=[id0, id3, id1])
    s.rekey(k2)
    assert s.engine.imported[-1] is k2 and (s.key_id, s.b_old, s.bit_levels) == (id2, 17, 3)
    assert s.old_generations == [(id0, 12), (id1, 17)] and s.generations == [(id0, 12), (id1, 17)]
    assert s.engine.bridge_slots() == [0, 2]                       # id3's slot was dropped
    assert s.append(*docs(3)) == 20
    assert s.generations == [(id0, 12), (id1, 17), (id2, 20)]
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 20, "ends": [12, 17], "slots": [0, 2], "Q": 2}
    s.search(q[0])
    assert s.engine.searches[-1] == {"B": 20, "ends": [12, 17], "slots": [0, 2], "Q": 1}
    # a single-bridge dict cannot follow while two old generations are resident
    with pytest.raises(ValueError, match="2 old generations"):
        s.rekey(fake_keys(3, bridge_from=id0))
    # a third rotation needs all three
    with pytest.raises(ValueError, match=id2):
        s.rekey(fake_keys(3, bridge_from=[id0, id1]))
    assert s.key_id == id2 and s.generations == [(id0, 12), (id1, 17), (id2, 20)]
    s.rekey(fake_keys(3, bridge_from=[id0, id1, id2]))
    assert s.old_generations == [(id0, 12), (id1, 17), (id2, 20)] and s.key_id == id3
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 20, "ends": [12, 17, 20], "slots": [0, 1, 2], "Q": 2}
    # load resets to one generation and frees the extra slots
    body, ids = s.body[:4].numpy().view(U), s.ids[:4].numpy().view(U)
    assert s.load(body, ids) == 4
    assert s.generations == [(id3, 4)] and (s.b_old, s.old_key_id) == (0, None) and s.engine.bridge_slots() == [0]
    s.search_many(q)
    assert s.engine.searches[-1] == {"B": 4, "b_old": 0, "Q": 2}


def test_multi_dict_with_one_resident_generation_runs_the_single_bridge(stub_server):
    """A multi-bridge dict on a store with one resident generation: that
    generation's key goes to slot 0 and search_seeded_queries(b_old=...) is
    still what is called; with nothing resident no bridge is needed."""
    from fheicp.stored import key_fingerprint
    id0, id1, id2 = (key_fingerprint(fake_keys(g)["ksk"]) for g in range(3))
    s = stub_server(fake_keys(1))
    s.rekey(fake_keys(2, bridge_from=[id0, id1]))                  # nothing resident
    assert s.generations == [] and s.engine.bridge_slots() == []
    s = stub_server(fake_keys(1))
    s.load(np.zeros((6, 16), U), np.arange(6, dtype=U))
    k2 = fake_keys(2, bridge_from=[id0, id1])
    s.rekey(k2)
    assert (s.b_old, s.old_key_id, s.key_id) == (6, id1, id2) and s.old_generations == [(id1, 6)]
    assert s.engine.bridge_slots() == [0]
    np.testing.assert_array_equal(s.engine.slots[0], k2["bridge_keys"][1])
    s.search_many(np.zeros((3, 16), np.float32))
    assert s.engine.searches[-1] == {"B": 6, "b_old": 6, "Q": 3}


def test_hub_keeps_its_one_old_generation_rule():
    from fheicp.stored import CorpusHub
    hub = CorpusHub()
    hub.tenants["a"] = object()
    with pytest.raises(ValueError, match="one old generation per tenant"):
        hub.rekey("a", fake_keys(2, bridge_from=["x", "y"]))


def test_eval_keys_file_carries_the_multi_bridge_entries(tmp_path, stub_server):
    from fheicp.engine import eval_keys_seeded
    from fheicp.query import load_eval_keys, save_eval_keys
    from fheicp.stored import key_fingerprint
    id0, id1 = (key_fingerprint(fake_keys(g)["ksk"]) for g in range(2))
    k2 = fake_keys(2, bridge_from=[id0, id1])
    path = str(tmp_path / "eval.npz")
    save_eval_keys(path, k2)
    got = load_eval_keys(path)                                      # plain arrays: allow_pickle=False
    assert set(got) == set(k2)
    for name in ("bridge_keys", "bridge_gadget", "ksk"):
        np.testing.assert_array_equal(got[name], k2[name])
    assert got["bridge_keys"].shape == (2, 4)
    assert [str(f) for f in got["bridge_from"]] == [id0, id1]
    assert eval_keys_seeded(got) is False
    # the seeded multi entries are plain arrays too and mark the dict's form
    sd = {"bsk_body": np.zeros(4, U), "ksk_body": np.zeros(4, U), "eval_mask_key": np.zeros(8, np.uint32),
          "bridge_key_bodies": np.arange(6, dtype=U).reshape(2, 3), "bridge_mask_keys": np.ones((2, 8), np.uint32),
          "bridge_gadget": np.array([7, 3]), "bridge_from": np.array([id0, id1])}
    save_eval_keys(path, sd)
    got_s = load_eval_keys(path)
    np.testing.assert_array_equal(got_s["bridge_key_bodies"], sd["bridge_key_bodies"])
    np.testing.assert_array_equal(got_s["bridge_mask_keys"], sd["bridge_mask_keys"])
    assert eval_keys_seeded(got_s) is True
    with pytest.raises(ValueError, match="mix the seeded and the full form"):
        eval_keys_seeded(dict(got_s, bridge_keys=np.zeros((2, 4), U)))
    with pytest.raises(ValueError, match="mix the seeded and the full form"):
        eval_keys_seeded({"bsk": np.zeros(4, U), "bridge_key_bodies": np.zeros((2, 3), U)})
    # a server rekeys from the loaded dict
    s = stub_server(fake_keys(0))
    s.load(np.zeros((3, 16), U), np.arange(3, dtype=U))
    s.rekey(fake_keys(1, bridge_from=id0))
    s.append(np.zeros((2, 16), U), np.arange(2, dtype=U))
    s.rekey(got)
    assert s.old_generations == [(id0, 3), (id1, 5)] and s.key_id == str(k2["key_id"][0])


# ------------------------------------------- the segmented bridge, restated --
def segmented_bridge_ref(ct, Q, B, ends, keys, beta, lv):
    """bridge_ref segment by segment: rows {q B + b : ends[g-1] <= b < ends[g]}
    with keys[g]; every other row unchanged. ct [Q B, kN+1]."""
    out = np.array(ct, dtype=U, copy=True)
    lo = 0
    for g, hi in enumerate(ends):
        idx = np.array([q * B + b for q in range(Q) for b in range(lo, hi)], dtype=np.int64)
        if idx.size:
            out[idx] = BR.bridge_ref(ct[idx], keys[g], beta, lv)
        lo = hi
    return out


def test_segmented_restatement_decrypts_under_the_new_secret():
    """TOY, three old secrets and one new: Q = 2, B = 11, ends [3, 3, 7, 9]
    (an empty generation; documents 9 and 10 current). Every row reads its
    message under the new secret after the segmented bridge, and a row bridged
    with another generation's key does not."""
    p = TOY
    big = p.k * p.N
    rng = np.random.default_rng(53)
    beta, lv = bridge_plan(p, 0.0)
    s_new = rng.integers(0, 2, big, dtype=U)
    s_olds = [rng.integers(0, 2, big, dtype=U) for _ in range(4)]
    keys = [BR.make_bridge_key(rng, s, s_new, beta, lv, p.glwe_noise_bits) for s in s_olds]
    Qn, B, ends = 2, 11, [3, 3, 7, 9]
    P = p.msg_bits
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), Qn * B)
    gen_of = lambda b: next((g for g, e in enumerate(ends) if b < e), None)  # noqa: E731
    ct = np.zeros((Qn * B, big + 1), U)
    for r in range(Qn * B):
        g = gen_of(r % B)
        ct[r] = BR.encrypt_lwe(rng, msgs[r:r + 1], s_new if g is None else s_olds[g], P, p.glwe_noise_bits)[0]
    out = segmented_bridge_ref(ct, Qn, B, ends, keys, beta, lv)
    np.testing.assert_array_equal(BR.decode(BR.lwe_phase(out, s_new), P), msgs)
    cur = np.array([r for r in range(Qn * B) if gen_of(r % B) is None])
    np.testing.assert_array_equal(out[cur], ct[cur])                # current-key rows untouched
    assert len(cur) == 4
    # the wrong generation's key does not decrypt
    wrong = segmented_bridge_ref(ct, Qn, B, ends, [keys[2], keys[1], keys[0], keys[3]], beta, lv)
    bad = BR.decode(BR.lwe_phase(wrong, s_new), P) != msgs
    old02 = np.array([gen_of(r % B) in (0, 2) for r in range(Qn * B)])
    assert bad[old02].mean() > 0.8 and not bad[~old02].any()
