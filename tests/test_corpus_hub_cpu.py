"""CPU: the group key switch and the stored-ciphertext hub,
the parts that need no GPU: header, library and binding agree on the new
entries; what the new entries refuse before they look at a group; and
CorpusHub's round forming and width rule as pure Python on EncryptedCorpus
planning objects. (A group cannot be created on host-only contexts,
fhe_group_create stops at their missing keys, so the per-tenant argument
order of the new entries is checked on the device, tests/test_gpu_corpus_hub.py.)"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from fheicp import _lib
from fheicp.corpus import CorpusQuant, EncryptedCorpus
from fheicp.model import QuantParams
from fheicp.params import TOY, params_for_bits

E_ARG = -1
HDR = (Path(__file__).resolve().parents[1] / "include" / "fhe_icp.h").read_text()


# ------------------------------------------------- header, library, binding --
def test_header_library_and_binding_agree():
    L = _lib.lib()
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name, nargs in (("fhe_group_form", 1), ("fhe_keyswitch_group_batch", 7),
                        ("fhe_search_seeded_queries_group_batch", 4)):
        decl = re.search(r"\bint " + name + r"\((.*?)\);", HDR, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(bound[name][1]), name
        assert getattr(L, name).argtypes == bound[name][1]
    body = re.search(r"typedef struct fhe_group_corpus \{(.*?)\} fhe_group_corpus;", HDR, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f for f, _ in _lib.FheGroupCorpus._fields_] and fields[0] == "struct_size"
    # the arguments of fhe_search_seeded_queries_bridged_batch, all of them
    assert set(fields) - {"struct_size", "reserved"} == {"d_body", "d_id0", "B", "D", "h_mask_key", "Q", "d_W", "cst",
                                                         "h_T", "levels_bit", "B_old", "d_glwe_acc", "d_glwe_bit"}
    assert C.sizeof(_lib.FheGroupCorpus) == 104


def test_group_form_follows_group_create():
    L = _lib.lib()
    form = lambda p: L.fhe_group_form(C.byref(_lib.params_struct(p.as_dict())))  # noqa: E731
    assert form(TOY) == 1
    assert all(form(params_for_bits(P)) == 1 for P in range(4, 27))
    assert form(params_for_bits(27)) == 0                       # a classic round: fhe_group_create refuses it
    bad = _lib.params_struct(TOY.as_dict())
    bad.struct_size -= 4
    assert L.fhe_group_form(C.byref(bad)) == E_ARG
    from fheicp.stored import group_form
    assert group_form(params_for_bits(27), 27) is False and group_form(TOY, 8) is True


def test_new_entries_reject_a_null_group():
    L = _lib.lib()
    c = (C.c_int64 * 1)(1)
    assert L.fhe_keyswitch_group_batch(None, None, c, 0, 0, None, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)
    assert L.fhe_search_seeded_queries_group_batch(None, None, 1, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)


# ------------------------------------------------ rounds and the width rule --
def toy_cq():
    """The 5-feature, 2-bit model of tests/test_gpu_group.py (P0 = 8)."""
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    return CorpusQuant(qp, 2, 0.5)


def wide_cq():
    """sum |q_w| = 2000 and 8-bit documents: P0 = 27, reached by a query of
    full-scale values; a query of small values plans far below it."""
    qp = QuantParams(n_bits=8, coef=np.array([500.0, -500.0, 500.0, -500.0]), intercept=0.0, s_x=1.0, zp_x=0,
                     s_w=1.0, q_w=np.array([500, -500, 500, -500], dtype=np.int64), q_b=0)
    return CorpusQuant(qp, 8, 1.0)


def covered(rounds):
    return sorted((p["name"], q) for r in rounds for p in r["parts"] for q in p["queries"])


def test_rounds_share_one_width_and_shift_exactly():
    from fheicp.stored import corpus_rounds
    cq = toy_cq()
    plans = {n: EncryptedCorpus(cq, TOY) for n in ("alice", "bob", "carol")}
    assert plans["alice"].P0 == 8
    big = np.array([[-1.0, 0.5, -1.0, 0.5, -1.0]] * 3, np.float32)       # full-scale values: the widest rows
    small = np.array([[0.5, 0.0, 0.0, 0.0, 0.0]], np.float32)
    mid = np.array([[0.5, 0.5, 0.0, 0.0, 0.5], [-1.0, 0.5, 0.0, 0.0, 0.0]], np.float32)
    requests = {"alice": (big, [None, 0.25, 0.5]), "bob": (small, 0.5), "carol": (mid, None)}
    sizes = {"alice": 130, "bob": 1, "carol": 17}
    rounds = corpus_rounds(requests, plans, sizes)
    assert [r["mode"] for r in rounds] == ["group"]
    (r,) = rounds
    assert [p["name"] for p in r["parts"]] == ["alice", "bob", "carol"]
    assert r["P"] == max(p["P_t"] for p in r["parts"]) <= 8
    assert min(p["P_t"] for p in r["parts"]) < r["P"], "the case must hold a tenant below the round's width"
    for p in r["parts"]:
        queries, ts = requests[p["name"]]
        Wr, cst, Ts, P_t = plans[p["name"]].plan_many(queries, ts)
        assert (P_t, cst, Ts) == (p["P_t"], p["cst"], p["Ts"])
        # the shifted rows times 2^(P - P_t) are the tenant's own: the shift dropped only zero bits
        np.testing.assert_array_equal(p["W"] * np.int64(2 ** (r["P"] - P_t)), Wr)
        # and they are the clear weights at the round's rescale 2^(P0 - P)
        W = np.stack([cq.weights(cq.quant(q)) for q in np.atleast_2d(queries)])
        np.testing.assert_array_equal(p["W"], W * np.int64(2 ** (8 - r["P"])))
    assert covered(rounds) == [("alice", 0), ("alice", 1), ("alice", 2), ("bob", 0), ("carol", 0), ("carol", 1)]


def test_lone_tenant_and_p27_fall_back_to_the_tenants_own_servers():
    from fheicp.stored import corpus_rounds
    cq = toy_cq()
    plan = EncryptedCorpus(cq, TOY)
    q = np.array([[0.5, 0.0, 0.5, 0.0, 0.5]], np.float32)
    rounds = corpus_rounds({"carol": (q, None)}, {"carol": plan}, {"carol": 17})
    assert [(r["mode"], len(r["parts"])) for r in rounds] == [("own", 1)]
    # P = 27: the round's width has no group form (a classic round), both tenants go through their own servers
    w = wide_cq()
    assert w.worst_msg_bits() == 27
    plans = {n: EncryptedCorpus(w) for n in ("alice", "bob")}
    assert plans["alice"].scheme == params_for_bits(27)
    full = np.array([[127.0, -128.0, 127.0, -128.0]], np.float32)
    tiny = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    rounds = corpus_rounds({"alice": (full, None), "bob": (tiny, None)}, plans, {"alice": 4, "bob": 4})
    (r,) = rounds
    assert r["P"] == 27 and r["mode"] == "own" and [p["P_t"] for p in r["parts"]][1] < 27
    # own-server parts keep their own rows: no shift was applied
    np.testing.assert_array_equal(r["parts"][1]["W"], plans["bob"].plan_many(tiny, None)[0])
    # the same tenants below 27 follow fhe_group_form at the round's width
    from fheicp.stored import group_form
    rounds = corpus_rounds({"alice": (tiny, None), "bob": (tiny, None)}, plans, {"alice": 4, "bob": 4})
    (r,) = rounds
    assert r["P"] < 27 and r["mode"] == ("group" if group_form(plans["alice"].scheme, r["P"]) else "own")
    # the choice is the predicate's
    rounds = corpus_rounds({"alice": (tiny, None), "bob": (tiny, None)}, plans, {"alice": 4, "bob": 4},
                           group_ok=lambda P: False)
    assert rounds[0]["mode"] == "own"


def test_rounds_follow_query_chunks_and_the_result_bound():
    from fheicp.query import query_chunks
    from fheicp.stored import corpus_rounds
    cq = toy_cq()
    plans = {n: EncryptedCorpus(cq, TOY) for n in ("bob", "alice")}
    rng = np.random.default_rng(3)
    requests = {"bob": (rng.uniform(-1, 0.5, (3, 5)), None), "alice": (rng.uniform(-1, 0.5, (10, 5)), 0.5)}
    sizes = {"bob": 10, "alice": 10}
    rounds = corpus_rounds(requests, plans, sizes, cap=80)
    assert covered(rounds) == sorted([("bob", q) for q in range(3)] + [("alice", q) for q in range(10)])
    assert all(sum(len(p["queries"]) * 10 for p in r["parts"]) <= 80 for r in rounds)
    # round 0 is chunk 0 of both (bob's 3 queries, alice's first 8, of which 5 fit beside bob's), then the
    # rest of alice's chunk 0 alone, then round 1: alice's chunk 1 alone
    assert [len(c) for c in query_chunks(10, 10, 80)] == [8, 2]
    shape = [(r["mode"], [(p["name"], p["queries"]) for p in r["parts"]]) for r in rounds]
    assert shape == [("group", [("bob", range(0, 3)), ("alice", range(0, 5))]),
                     ("own", [("alice", range(5, 8))]),
                     ("own", [("alice", range(8, 10))])]
    # a tenant's queries stay in order across the rounds
    assert [q for r in rounds for p in r["parts"] if p["name"] == "alice" for q in p["queries"]] == list(range(10))


# ---------------------------------------------------------------- CorpusHub --
class StubServer:
    def __init__(self, P0, scheme):
        self.P0, self.scheme, self.body = P0, scheme, None


def test_hub_refuses_another_p0_by_name():
    from fheicp.stored import CorpusHub
    hub = CorpusHub()
    hub.add_tenant("alice", None, None, 8, None, server=StubServer(8, TOY))
    hub.add_tenant("bob", None, None, 8, None, server=StubServer(8, TOY))
    with pytest.raises(ValueError, match="'carol'.*P0 = 27"):
        hub.add_tenant("carol", None, None, 27, None, server=StubServer(27, params_for_bits(27)))
    # refused before any server is built from the keys (there is no GPU here)
    with pytest.raises(ValueError, match="'carol'.*P0 = 27"):
        hub.add_tenant("carol", {}, wide_cq(), 27, np.zeros(8, np.uint32))
    with pytest.raises(ValueError, match="'carol'.*worst-case width 8"):
        hub.add_tenant("carol", {}, toy_cq(), 12, np.zeros(8, np.uint32), scheme=TOY)
    with pytest.raises(ValueError, match="'dave'.*scheme"):
        hub.add_tenant("dave", None, None, 8, None, server=StubServer(8, params_for_bits(8)))
    with pytest.raises(ValueError, match="'bob'.*already"):
        hub.add_tenant("bob", None, None, 8, None, server=StubServer(8, TOY))
    assert list(hub.tenants) == ["alice", "bob"]
    with pytest.raises(ValueError, match="unknown tenant 'erin'"):
        hub.search_many({"erin": ([], None)})
    with pytest.raises(ValueError, match="'alice' has no documents"):
        hub.search_many({"alice": (np.zeros((1, 5)), None)})
