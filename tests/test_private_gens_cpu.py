"""CPU: both-private key rotation without a device.

The numpy restatement decodes (per generation the external product under that
generation's key, then the bridge on the old generations' rows: every row opens
under the NEWEST key to the clear accumulator); params.private_rotation_plan
reproduces the design's table; the two library entries report argument errors
on host-only contexts before the missing device; PrivateServer's bundle and
rekey checks on a stub engine."""
import ctypes as C
import math

import numpy as np
import pytest

import bridge_ref as BR
import private_gens_ref as PG

from fheicp import _lib
from fheicp.params import (TOY, bridge_var, extprod_plan, extprod_var, pack_plan, pack_sigmas, params_for_bits,
                           private_rotation_plan)

U = np.uint64


# ----------------------------------------------------------- restatement --
def test_restatement_decodes_under_the_newest_key():
    """Three generations on TOY, D = 5, B = [7, 1, 3], Q = 2, gadget (7, 4)
    for the product and the bridge: generation g's documents under s_g meet
    generation g's GGSWs under s_g; the rows of generations 0 and 1 are
    bridged with keys s_0 -> s_2 and s_1 -> s_2. Every row's phase under s_2
    decodes to sum_j W_j dq[b, j] + cst; the current generation's rows are the
    product's own words; an old generation's row does NOT decode under s_2
    before its bridge."""
    p = TOY
    N, k, P, nb = p.N, p.k, p.msg_bits, p.glwe_noise_bits
    beta, L = 7, 4
    rng = np.random.default_rng(819)
    Bs, D, Qn = [7, 1, 3], 5, 2
    s = [rng.integers(0, 2, k * N, dtype=U) for _ in Bs]
    dq = [rng.integers(-2, 2, (B, D)) for B in Bs]
    W = rng.integers(-2, 3, (Qn, D))
    csts = [3, -5]
    glwes = [PG.encrypt_docs_glwe(rng, dq[g], s[g], N, k, P, nb) for g in range(3)]
    ggsws = [np.stack([PG.encrypt_ggsw(rng, W[q], s[g], N, k, beta, L, nb) for q in range(Qn)]) for g in range(3)]
    rows = PG.linear_gens_ref(glwes, ggsws, Bs, beta, D, csts, P)
    B = sum(Bs)
    assert rows.shape == (Qn * B, k * N + 1)
    keys = [BR.make_bridge_key(rng, s[g], s[2], beta, L, nb) for g in (0, 1)] + [None]
    out = PG.bridge_gens_ref(rows, Qn, Bs, keys, beta, L)
    want = np.concatenate([np.concatenate([dq[g] @ W[q] + csts[q] for g in range(3)]) for q in range(Qn)])
    assert np.abs(want).max() < 2 ** (P - 1)
    np.testing.assert_array_equal(BR.decode(BR.lwe_phase(out, s[2]), P), want)
    cur = PG.gen_rows(Qn, Bs, 2)
    np.testing.assert_array_equal(out[cur], rows[cur])                 # current-generation rows untouched
    for g in (0, 1):
        idx = PG.gen_rows(Qn, Bs, g)
        assert not np.array_equal(out[idx], rows[idx])
        np.testing.assert_array_equal(BR.decode(BR.lwe_phase(rows[idx], s[g]), P), want[idx])   # its own key opens it
        assert not np.array_equal(BR.decode(BR.lwe_phase(rows[idx], s[2]), P), want[idx])       # the new one does not
    # the row layout: q B + off_g + b
    assert PG.offsets(Bs) == [0, 7, 8]
    assert list(PG.gen_rows(Qn, Bs, 1)) == [7, 18] and list(PG.gen_rows(Qn, Bs, 2)) == [8, 9, 10, 19, 20, 21]


# ------------------------------------------------------------------ plan --
# DESIGN.md §8.19's table: P0, log2 ||W||^2, GGSW gadget, bridge gadget, margin before and after the bridge,
# the packing plan after it and its margin
TABLE = [(16, 27, (7, 6), (7, 4), 313.0, 181.0, (7, 4, 2), 140.0),
         (21, 27, (7, 6), (7, 5), 9.79, 9.79, (7, 5, 2), 9.79),
         (23, 29, (7, 7), (7, 5), 152.0, 125.0, (7, 5, 2), 81.0),
         (27, 27, (7, 7), (7, 5), 18.9, 11.2, (5, 8, 2), 10.1)]


def agree_to_two_figures(x: float, table: float) -> bool:
    """Within half a unit of the table value's second significant figure."""
    return abs(x - table) <= 0.5 * 10.0 ** (math.floor(math.log10(table)) - 1)


@pytest.mark.parametrize("P0,lw,ggsw,bridge,before,after,pack,pack_margin", TABLE, ids=[f"P{r[0]}" for r in TABLE])
def test_rotation_plan_reproduces_the_table(P0, lw, ggsw, bridge, before, after, pack, pack_margin):
    p = params_for_bits(P0).with_msg_bits(P0)
    w2 = 2.0 ** lw
    g, bg, in_var = private_rotation_plan(p, w2)
    assert g == ggsw == extprod_plan(p, w2)        # documents packed before a rotation stay valid after it
    assert bg == bridge
    ev, bv = extprod_var(p, w2, *g), bridge_var(p, *bg)
    assert in_var == (ev + bv) / 2.0 ** 128
    m = 2.0 ** (63 - P0)
    assert agree_to_two_figures(m / math.sqrt(ev), before)
    assert agree_to_two_figures(m / math.sqrt(ev + bv), after)
    assert m / math.sqrt(ev + bv) >= 9.2
    plan = pack_plan(p, 1024, in_var)
    assert plan == pack
    assert agree_to_two_figures(pack_sigmas(p, 1024, in_var, plan[0], plan[1], 63 - P0), pack_margin)


def test_rotation_plan_equals_plan_gadget_and_refuses():
    """The GGSW gadget is plan_gadget's on a real model; a norm no int8
    gadget carries raises plan_gadget's wording."""
    from fheicp.private import plan_gadget, worst_norm2

    class M:
        q_w = np.array([3, -2, 5, 1, -4, 2, 2, -1] * 2)

    class CQ:
        model, n_e = M(), 6

    p = params_for_bits(21).with_msg_bits(21)
    g, bg, _ = private_rotation_plan(p, worst_norm2(CQ()))
    assert g == plan_gadget(p, CQ())
    with pytest.raises(ValueError, match="no GGSW gadget at P0 = 27"):
        private_rotation_plan(params_for_bits(27).with_msg_bits(27), 2.0 ** 60)


def largest_norm_of_first_gadget(p, start: float):
    """The largest ||W||^2 (to the last float) for which extprod_plan still
    picks the gadget it picks at `start`: its margin sits at 9.2 there."""
    base = extprod_plan(p, start)
    lo, hi = start, start * 2.0 ** 20
    for _ in range(200):
        mid = (lo + hi) / 2
        if extprod_plan(p, mid) == base:
            lo = mid
        else:
            hi = mid
    return base, lo


def test_rotation_plan_steps_when_only_the_bridge_term_fails():
    """At the norm where extprod_plan's gadget sits exactly at 9.2 sigma, the
    bridge's added variance takes it below: at P0 = 21 the plan steps from
    (7, 6) to the next gadget of extprod_plan's order, (7, 7), and passes
    there; at P0 = 23 the gadget is already the last one that can pass, so the
    plan refuses although extprod_plan alone does not."""
    p = params_for_bits(21).with_msg_bits(21)
    base, w2 = largest_norm_of_first_gadget(p, 2.0 ** 27)
    assert base == (7, 6)
    m = 2.0 ** (63 - 21)
    ev = extprod_var(p, w2, *base)
    assert m / math.sqrt(ev) >= 9.2 > m / math.sqrt(ev + bridge_var(p, 7, 5))
    g, bg, in_var = private_rotation_plan(p, w2)
    assert g == (7, 7) and g != extprod_plan(p, w2)
    assert m / math.sqrt(in_var * 2.0 ** 128) >= 9.2
    assert in_var == (extprod_var(p, w2, *g) + bridge_var(p, *bg)) / 2.0 ** 128
    p23 = params_for_bits(23).with_msg_bits(23)
    base23, w23 = largest_norm_of_first_gadget(p23, 2.0 ** 29)
    assert base23 == (7, 7) == extprod_plan(p23, w23)
    with pytest.raises(ValueError, match="no GGSW gadget at P0 = 23"):
        private_rotation_plan(p23, w23)


# -------------------------------------------------- host-only contexts --
def gens_array(specs):
    """specs: (struct_size or None, slot, d_ggsw, d_docs, B) -> (FheGgswGen array, G)."""
    arr = (_lib.FheGgswGen * max(1, len(specs)))()
    for i, (size, slot, g, d, B) in enumerate(specs):
        arr[i].struct_size = C.sizeof(_lib.FheGgswGen) if size is None else size
        arr[i].slot, arr[i].d_ggsw, arr[i].d_docs, arr[i].B = slot, g, d, B
    return arr


def test_gens_entry_points_on_host_context():
    """FHE_E_ARG first, each before the device error; a well-formed call then
    reports the host-only context."""
    L = _lib.lib()
    prm = params_for_bits(21)
    P = _lib.params_struct(prm.as_dict())
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(P), -1, C.byref(h)) == 0
    buf = (C.c_uint64 * 64)()      # stands for every device buffer: nothing reads it on a host-only context
    bp = C.addressof(buf)
    hv = (C.c_int64 * 4)()

    def lin(specs, G=None, Q=2, D=16, b=7, lv=6, hc=hv, out=buf):
        return L.fhe_linear_ggsws_gens_batch(h, C.byref(gens_array(specs)), len(specs) if G is None else G, b, lv, Q, D,
                                             hc, out, None)

    def sea(specs, G=None, Q=2, D=16, b=7, lv=6, hc=hv, out=buf, lb=0):
        return L.fhe_search_ggsws_gens_batch(h, C.byref(gens_array(specs)), len(specs) if G is None else G, b, lv, Q, D,
                                             0, hc, lb, out, buf, None)

    good = [(None, 3, bp, bp, 5), (None, 0, bp, bp, 0), (None, -1, bp, bp, 4)]
    for f in (lin, sea):
        def bad(match, *a, **kw):
            assert f(*a, **kw) == -1, (match, a, kw)
            assert match in L.fhe_last_error(h), (match, L.fhe_last_error(h))
        bad(b"struct_size", [(8, 0, bp, bp, 5)])
        bad(b"G outside", good, G=0)
        bad(b"G outside", good * 4, G=10)
        bad(b"named twice", [(None, 2, bp, bp, 5), (None, 2, bp, bp, 1)])
        bad(b"must be the last", [(None, -1, bp, bp, 5), (None, 2, bp, bp, 1)])
        bad(b"outside [0, 8)", [(None, 8, bp, bp, 5)])
        bad(b"outside [0, 8)", [(None, -2, bp, bp, 5)])
        bad(b"no generation holds a document", [(None, 0, bp, bp, 0), (None, -1, None, None, 0)])
        bad(b"null", [(None, 0, None, bp, 5)])
        bad(b"null", [(None, 0, bp, None, 5)])
        bad(b"B outside", [(None, 0, bp, bp, -1)])
        bad(b"D > N", good, D=prm.N + 1)
        bad(b"gadget out of range", good, b=8)
        bad(b"gadget out of range", good, lv=9)
        bad(b"Q < 1", good, Q=0)
        bad(b"null", good, hc=None)
        bad(b"null", good, out=None)
        assert f(good) == -2 and b"host-only" in L.fhe_last_error(h)
        # an empty generation's pointers are ignored; old generations only is allowed
        assert f([(None, 1, None, None, 0), (None, 4, bp, bp, 3)]) == -2
        # nine generations, eight slots and the current key
        assert f([(None, s, bp, bp, 1) for s in range(8)] + [(None, -1, bp, bp, 1)]) == -2
    for lb in (9, -1):
        assert sea(good, lb=lb) == -1 and b"levels_bit" in L.fhe_last_error(h)
    assert L.fhe_linear_ggsws_gens_batch(None, C.byref(gens_array(good)), 3, 7, 6, 2, 16, hv, buf, None) == -1
    assert L.fhe_linear_ggsws_gens_batch(h, None, 3, 7, 6, 2, 16, hv, buf, None) == -1
    L.fhe_ctx_destroy(h)


def test_gens_workspace_bytes():
    """G = 1: the sibling's bytes. Several generations: each one's planes and
    result, the Q constants once; an empty generation adds nothing."""
    L = _lib.lib()
    prm = params_for_bits(21)
    P = _lib.params_struct(prm.as_dict())

    def gens(Qn, Bs, D=16, lv=6):
        a = (C.c_int64 * len(Bs))(*Bs)
        return L.fhe_ggsws_gens_ws_bytes(C.byref(P), Qn, a, len(Bs), D, lv)

    def one(Qn, B, D=16, lv=6):
        return L.fhe_ggsws_ws_bytes(C.byref(P), Qn, B, D, lv)

    for Qn, B in ((1, 1), (8, 128), (8, 1024), (11, 300)):
        assert gens(Qn, [B]) == one(Qn, B) > 0
    assert gens(8, [64, 0, 500]) == one(8, 64) + one(8, 500) - 8 * 8 == gens(8, [64, 500])
    assert gens(8, [0, 0]) == 0 and gens(8, [4, -1]) == 0 and gens(0, [4]) == 0 and gens(8, [4], D=0) == 0
    assert gens(8, [1] * 10) == 0 and gens(8, [4], lv=9) == 0
    assert L.fhe_ggsws_gens_ws_bytes(C.byref(P), 8, None, 1, 16, 6) == 0


# -------------------------------------------------------- bundle handling --
class StubEngine:
    """What PrivateServer's store touches of an Engine before the search call."""

    def __init__(self):
        self.slots, self.imported, self.dropped = [], [], []

    def bridge_slots(self):
        return sorted(self.slots)

    def drop_bridge_key(self, s):
        self.slots.remove(s)
        self.dropped.append(s)

    def import_eval_keys(self, d):
        self.imported.append(d)
        n = len(np.asarray(d["bridge_from"]).reshape(-1)) if "bridge_from" in d else 0
        self.slots = list(range(n))


class StubModel:
    q_w = np.array([2, -1, 2, -2, 1])


class StubQuant:
    model, n_e, q_b = StubModel(), 2, 0


def stub_server(key_id="gen0", blocks=()):
    """A PrivateServer on a stub engine with `blocks` (key_id, B) resident."""
    from fheicp.private import PrivateServer
    s = PrivateServer.__new__(PrivateServer)
    s.cq, s.P0, s.scheme = StubQuant(), 8, TOY
    s.base_log, s.level, s.bit_levels = 4, 3, 0
    s.engine = StubEngine()
    s._seeded_docs = {}
    s._init_store({"key_id": np.array([key_id])})
    s._gens = [{"key_id": k, "docs": None, "B": B} for k, B in blocks]
    return s


def full_payload(**over):
    from fheicp.private import pack_ggsw_query
    f = dict(D=5, P0=8, base_log=4, level=3, N=TOY.N, k=TOY.k)
    f.update(over)
    words = (f["k"] + 1) * f["level"] * (f["k"] + 1) * f["N"]
    return pack_ggsw_query(np.zeros(words, U), f["D"], f["P0"], f["base_log"], f["level"], f["N"], f["k"])


def seeded_payload(id0=0):
    from fheicp.private import pack_ggsw_query_seeded
    return pack_ggsw_query_seeded(np.zeros((TOY.k + 1) * 3 * TOY.N, U), id0, np.arange(8, dtype=np.uint32), 5, 8, 4, 3,
                                  TOY.N, TOY.k)


def test_search_resident_refuses_before_any_device_work():
    s = stub_server("gen1", [("gen0", 20), ("gen1", 3)])
    assert s.generations == [("gen0", 20), ("gen1", 23)] and s.old_generations == [("gen0", 20)]
    two = [full_payload(), full_payload()]
    with pytest.raises(ValueError, match="documents under key gen0 are resident and the bundle holds no queries"):
        s.search_resident({"gen1": two})
    with pytest.raises(ValueError, match="generation gen0: query 1: a seeded payload in a batch of full-form"):
        s.search_resident({"gen0": [full_payload(), seeded_payload()], "gen1": two})
    with pytest.raises(ValueError, match="generation gen1: query 0: gadget differs"):
        s.search_resident({"gen0": two, "gen1": [full_payload(base_log=5), full_payload(base_log=5)]})
    with pytest.raises(ValueError, match="generation gen1: 1 queries, generation gen0 2"):
        s.search_resident({"gen0": two, "gen1": two[:1]})
    with pytest.raises(ValueError, match="generation gen0: query 0 was encrypted under different parameters"):
        s.search_resident({"gen0": [full_payload(P0=7)], "gen1": two})
    with pytest.raises(RuntimeError, match="no resident documents"):
        stub_server().search_resident({"gen0": two})
    assert s.engine.imported == [] and s.engine.dropped == []


def rotated_keys(key_id, src, single=False):
    d = {"pack_key": np.zeros(1, U), "key_id": np.array([key_id]), "bridge_gadget": np.array([4, 3]),
         "bridge_from": np.array(src), "pack_bit_levels": np.array([2])}
    d["bridge_key" if single else "bridge_keys"] = np.zeros((len(src), 4), U)
    return d


def test_rekey_needs_a_bridge_from_every_resident_generation():
    s = stub_server("gen1", [("gen0", 20), ("gen1", 3)])
    s._slots = {"gen0": 0}
    s.engine.slots = [0]
    before = (list(s._gens), dict(s._slots), s.key_id, s.bit_levels)
    for keys in (rotated_keys("gen2", ["gen1"]), rotated_keys("gen2", ["gen1"], single=True),
                 {"pack_key": np.zeros(1, U), "key_id": np.array(["gen2"])}):
        with pytest.raises(ValueError, match="documents under key gen0 are resident and the evaluation keys hold no "
                                             "bridge key from it"):
            s.rekey(keys)
        assert (s._gens, s._slots, s.key_id, s.bit_levels) == before and s.engine.imported == []
    with pytest.raises(ValueError, match="no packing key"):
        s.rekey({"bridge_keys": np.zeros((1, 4), U)})
    with pytest.raises(ValueError, match="no bridge_from"):
        s.rekey({"pack_key": np.zeros(1, U), "bridge_keys": np.zeros((1, 4), U)})
    # a complete set, with a bridge from a generation that is not resident: its slot is dropped
    s.rekey(rotated_keys("gen2", ["gone", "gen0", "gen1"]))
    assert s.key_id == "gen2" and s._slots == {"gen0": 1, "gen1": 2} and s.bit_levels == 2
    assert s.engine.dropped == [0] and s.engine.bridge_slots() == [1, 2]
    assert s.generations == [("gen0", 20), ("gen1", 23)] == s.old_generations
    # the single-bridge dict on a store of one generation
    t = stub_server("gen0", [("gen0", 4)])
    t.rekey(rotated_keys("gen1", ["gen0"], single=True))
    assert t.key_id == "gen1" and t._slots == {"gen0": 0} and t.old_generations == [("gen0", 4)]


def test_append_continues_a_generation_only_at_a_glwe_boundary():
    s = stub_server("gen1", [("gen0", 20), ("gen1", 3)])          # S = 256 // 5 = 51 documents per GLWE
    with pytest.raises(ValueError, match="GLWE boundary"):
        s.append(np.zeros(8, U))
