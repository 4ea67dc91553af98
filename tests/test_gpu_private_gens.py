"""GPU: both-private key rotation through libfheicp.

fhe_linear_ggsws_gens_batch word for word against fhe_linear_ggsws_batch per
generation (and the numpy restatement, tests/private_gens_ref.py) over the
shapes where the grouped launch takes another path; fhe_search_ggsws_gens_batch
against the entries it is composed of; an evaluation-only PrivateServer that
lives through two rotations answers what the clear restatement answers, in both
payload forms; and the bridged rows' noise at the real P0 = 21 parameters."""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import private_gens_ref as PG
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine, u64
from fheicp.params import TOY, bridge_var, extprod_var, params_for_bits, private_rotation_plan

pytestmark = pytest.mark.gpu

U = np.uint64
CANARY = 0x5EA15EA15EA15EA1
BETA, LV = 4, 3                            # the product's and the bridge's gadget on TOY
PERM8 = [3, 7, 0, 5, 1, 6, 2, 4]           # old generation g -> bridge slot: not the identity
CSTS = [-37, 5, 0, 11, -1, 300, -4096, 2, 7, -8, 1]
# the product library runs the grouped product; the per-generation loop exists as an A/B build only
GROUPED = Path(_lib.LIB_PATH).name == "libfheicp.so"


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def slots_for(Bs, current_last=True):
    """Old generation g in slot PERM8[g]; the last generation under the current key."""
    return [PERM8[g] for g in range(len(Bs) - 1)] + [-1 if current_last else PERM8[len(Bs) - 1]]


@pytest.fixture(scope="module")
def toy(need_gpu):
    """A TOY context with keys, a packing key and eight numpy-made bridge keys
    of uniform words, gadget (4, 3): keys[g] sits in slot PERM8[g]."""
    eng = Engine(TOY, 0)
    eng.keygen(99)
    eng.keygen_pack(7, 3, seed=5)
    rng = np.random.default_rng(2025)
    big = TOY.k * TOY.N
    keys = [rng.integers(0, 2 ** 64, (big, LV, big + 1), dtype=U) for _ in range(8)]
    for g, bk in enumerate(keys):
        eng.import_bridge_key(BETA, LV, bk, slot=PERM8[g])
    yield eng, keys
    eng.close()


def random_operands(eng, rng, Qn, D, Bs):
    """Per generation: Q GGSWs and the document GLWEs of arbitrary words (the
    product is exact modulo 2^64 on any words), the packed operand and B."""
    p = eng.params
    gens = []
    for Bg in Bs:
        if Bg == 0:
            gens.append((None, None, None, 0))
            continue
        ggsws = rng.integers(0, 2 ** 64, (Qn, p.k + 1, LV, p.k + 1, p.N), dtype=U)
        glwe = rng.integers(0, 2 ** 64, (eng.doc_glwes(Bg, D), p.k + 1, p.N), dtype=U)
        docs = eng.pack_docs_glwe_queries(dev_u64(eng, glwe), Bg, D, BETA, LV)
        gens.append((ggsws, glwe, docs, Bg))
    return gens


# (Q, D, B per generation, compare with the numpy restatement too)
LINEAR_CASES = [
    (1, 16, [17, 1, 5], True),              # one row tile; a partial second GLWE
    (6, 5, [52, 0, 3, 51], False),          # 18 product rows: two row tiles and padding; an empty generation; S = 51
    (11, 256, [2, 1], False),               # four padded row tiles; S = 1
    (1, 256, [100, 40], False),             # 140 GLWEs: the K split is off
    (2, 16, [1] * 9, True),                 # nine segments
]


@pytest.mark.parametrize("Qn,D,Bs,numpy_too", LINEAR_CASES, ids=[f"q{c[0]}d{c[1]}g{len(c[2])}" for c in LINEAR_CASES])
def test_linear_gens_bit_exact(toy, Qn, D, Bs, numpy_too):
    """Row q B + off_g + b equals row q B_g + b of fhe_linear_ggsws_batch on
    generation g's operands, word for word; the row after Q B keeps its
    canary; one "linear_ggsws" bracket whatever G."""
    eng, _ = toy
    p = eng.params
    rng = np.random.default_rng(1000 * Qn + D + len(Bs))
    gens = random_operands(eng, rng, Qn, D, Bs)
    B = sum(Bs)
    csts = CSTS[:Qn]
    slots = slots_for(Bs)
    items = [(slots[g], None if gg is None else dev_u64(eng, gg), docs, Bg) for g, (gg, _, docs, Bg) in enumerate(gens)]
    buf = torch.full((Qn * B + 1, eng.W), CANARY, dtype=torch.int64, device=eng.device)
    eng.profile(True)
    try:
        out = eng.linear_ggsws_gens(items, BETA, LV, D, csts, out=buf)
        prof = eng.profile_read("linear_ggsws")
    finally:
        eng.profile(False)
    assert out.data_ptr() == buf.data_ptr()
    got = u64(buf)
    assert (got[Qn * B] == U(CANARY)).all()
    if GROUPED:
        assert (prof["launches"], prof["items"]) == (1, Qn * B)
        assert eng.kernel_name("linear_ggsws") == f"k_extprod_queries_mfma_grp<{1 if 3 * Qn <= 16 else 2}>"
    per = []
    for g, (gg, glwe, docs, Bg) in enumerate(gens):
        per.append(None if Bg == 0 else u64(eng.linear_ggsws(items[g][1], BETA, LV, docs, Bg, D, csts)))
    want = PG.scatter_gens(per, Qn, Bs, eng.W)
    np.testing.assert_array_equal(got[:Qn * B], want)
    assert eng.ggsws_gens_ws_bytes(Qn, Bs, D, LV) == sum(eng.ggsws_ws_bytes(Qn, b, D, LV) - 8 * Qn for b in Bs if b) + 8 * Qn
    if numpy_too:
        ref = PG.linear_gens_ref([g[1] for g in gens], [g[0] for g in gens], Bs, BETA, D, csts, p.msg_bits)
        np.testing.assert_array_equal(got[:Qn * B], ref)


def test_linear_gens_old_generations_only(toy):
    """No slot -1 entry: the same rows."""
    eng, _ = toy
    Qn, D, Bs = 3, 5, [4, 60]
    gens = random_operands(eng, np.random.default_rng(4), Qn, D, Bs)
    items = [(s, dev_u64(eng, gg), docs, Bg) for s, (gg, _, docs, Bg) in zip(slots_for(Bs, False), gens)]
    got = u64(eng.linear_ggsws_gens(items, BETA, LV, D, CSTS[:Qn]))
    per = [u64(eng.linear_ggsws(it[1], BETA, LV, it[2], it[3], D, CSTS[:Qn])) for it in items]
    np.testing.assert_array_equal(got, PG.scatter_gens(per, Qn, Bs, eng.W))


@pytest.mark.parametrize("Qn,D,B,rt", [
    (6, 5, 55, 2),      # 18 product rows: RT = 2 with padded rows; S = 51, a partial second GLWE; K split, atomics
    (1, 256, 140, 1),   # RT = 1; 140 GLWEs, 280 tiles: the K split is off, plain stores
], ids=["q6d5b55", "q1d256b140"])
def test_context_entry_is_the_group_entry_of_one_tenant(toy, Qn, D, B, rt):
    """The two callers of the segmented launcher agree: one generation under
    slot -1 through fhe_linear_ggsws_gens_batch, and a group of this one
    context through fhe_linear_ggsws_group_batch, on the same GGSWs, documents
    and constants. The first Q B rows are equal words; the context entry's row
    Q B keeps its canary, the group's rows from Q B on (its padding up to M and
    four more) their sentinel."""
    from fheicp.engine import EngineGroup, group_rows
    eng, _ = toy
    (ggsws, _, docs, _), = random_operands(eng, np.random.default_rng(24 * Qn + D), Qn, D, [B])
    gg = dev_u64(eng, ggsws)
    csts = CSTS[:Qn]
    n = Qn * B
    M, starts = group_rows([n])
    assert starts == [0] and M >= n
    a = torch.full((n + 1, eng.W), CANARY, dtype=torch.int64, device=eng.device)
    b = torch.full((M + 4, eng.W), CANARY + 1, dtype=torch.int64, device=eng.device)
    eng.linear_ggsws_gens([(-1, gg, docs, B)], BETA, LV, D, csts, out=a)
    if GROUPED:
        assert eng.kernel_name("linear_ggsws") == f"k_extprod_queries_mfma_grp<{rt}>"
    grp = EngineGroup([eng])
    try:
        grp.linear_ggsws([(gg.reshape(-1), BETA, LV, docs, B, D)], [csts], out=b)
        assert eng.kernel_name("linear_ggsws") == f"k_extprod_queries_mfma_grp<{rt}>"
        torch.cuda.synchronize()
    finally:
        grp.close()
    ga, gb = u64(a), u64(b)
    assert np.array_equal(ga[:n], gb[:n])
    assert (ga[:n, -1] != U(CANARY)).any()                             # the rows were written
    assert (ga[n] == U(CANARY)).all()
    assert (gb[n:] == U(CANARY + 1)).all()


# ----------------------------------------------------------- search entry --
def encrypted_operands(eng, rng, Qn, D, Bs):
    """Valid encryptions under the context's own key: the search entry's sign
    extraction then runs on phases it was made for."""
    gens = []
    for g, Bg in enumerate(Bs):
        W = rng.integers(-3, 4, (Qn, D))
        ggsws = torch.cat([eng.encrypt_ggsw(W[q], BETA, LV, 70 + g, id0=1000 * q).reshape(-1) for q in range(Qn)])
        glwe = eng.encrypt_docs_glwe(rng.integers(-2, 2, (Bg, D)), 80 + g, id0=0)
        gens.append((ggsws.contiguous(), eng.pack_docs_glwe_queries(glwe, Bg, D, BETA, LV), Bg))
    return gens


def test_search_gens_one_current_generation_is_search_ggsws(toy):
    """G = 1, slot -1: fhe_search_ggsws_batch word for word."""
    eng, _ = toy
    Qn, D, B = 3, 5, 60
    (ggsws, docs, _), = encrypted_operands(eng, np.random.default_rng(1), Qn, D, [B])
    Ts = [-3, 0, 4]
    ga, gb = eng.search_ggsws(ggsws, BETA, LV, docs, B, D, 2, Ts, 2)
    ga2, gb2 = eng.search_ggsws_gens([(-1, ggsws, docs, B)], BETA, LV, D, 2, Ts, 2)
    torch.cuda.synchronize()
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)


def composed_search(eng, items, Qn, D, cst, Ts, levels_bit, ends, slots):
    """The entries the search entry is composed of: the leveled step with
    cst - T_q (one generation: fhe_linear_ggsws_batch itself), the bridge
    over the old generations' rows, the copy, the sign extraction and the two
    packings."""
    B = sum(it[3] for it in items)
    if len(items) == 1:
        rows = eng.linear_ggsws(items[0][1], BETA, LV, items[0][2], B, D, [cst - t for t in Ts])
    else:
        rows = eng.linear_ggsws_gens(items, BETA, LV, D, [cst - t for t in Ts])
    if len(ends) == 1 and slots == [0]:
        eng.bridge_rows(rows, Qn, B, ends[0])
    else:
        eng.bridge_gens(rows, Qn, B, ends, slots)
    cpy = rows.clone()
    sgn = eng.sign(rows)
    return eng.pack(cpy, Qn * B, 0), eng.pack(sgn, Qn * B, levels_bit)


def test_search_gens_one_old_generation_in_slot_0(toy):
    """G = 1, slot 0: linear, fhe_bridge_rows_batch(B_old = B), fhe_sign_batch
    and fhe_pack_batch, word for word."""
    eng, _ = toy
    Qn, D, B = 2, 5, 55
    (ggsws, docs, _), = encrypted_operands(eng, np.random.default_rng(2), Qn, D, [B])
    Ts = [1, -2]
    items = [(0, ggsws, docs, B)]
    ga, gb = eng.search_ggsws_gens(items, BETA, LV, D, 3, Ts, 2)
    wa, wb = composed_search(eng, [(-1, ggsws, docs, B)], Qn, D, 3, Ts, 2, [B], [0])
    torch.cuda.synchronize()
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
    ga0, _ = eng.search_ggsws(ggsws, BETA, LV, docs, B, D, 3, Ts, 2)
    assert not torch.equal(ga, ga0)                                     # the bridge did something


def test_search_gens_three_generations_and_profile_brackets(toy):
    """Two old generations in slots 3 and 7 and the current one: the composed
    entries word for word, and exactly one "linear_ggsws" and one "bridge"
    bracket for the call."""
    eng, _ = toy
    Qn, D, Bs = 3, 5, [52, 3, 20]
    gens = encrypted_operands(eng, np.random.default_rng(3), Qn, D, Bs)
    slots = slots_for(Bs)
    items = [(s, gg, docs, Bg) for s, (gg, docs, Bg) in zip(slots, gens)]
    Ts = [0, 5, -5]
    eng.profile(True)
    try:
        ga, gb = eng.search_ggsws_gens(items, BETA, LV, D, 1, Ts, 0)
        lin, br = eng.profile_read("linear_ggsws"), eng.profile_read("bridge")
    finally:
        eng.profile(False)
    if GROUPED:
        assert (lin["launches"], lin["items"]) == (1, Qn * sum(Bs))
        assert (br["launches"], br["items"]) == (1, Qn * (Bs[0] + Bs[1]))
    wa, wb = composed_search(eng, items, Qn, D, 1, Ts, 0, [52, 55], slots[:2])
    torch.cuda.synchronize()
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
    # a named slot with rows and no key: FHE_E_STATE naming the slot, before anything is queued
    eng.drop_bridge_key(2)
    try:
        with pytest.raises(_lib.FheError, match="FHE_E_STATE.*no bridge key in slot 2"):
            eng.search_ggsws_gens([(2, *gens[0])], BETA, LV, D, 1, Ts, 0)
    finally:
        eng.import_bridge_key(BETA, LV, toy[1][PERM8.index(2)], slot=2)


# ------------------------------------------------------------ end to end --
def toy_model():
    """tests/test_gpu_private_hub.py's 5-feature, 2-bit model (P0 = 8)."""
    from fheicp.corpus import CorpusQuant
    from fheicp.model import QuantParams
    qp = QuantParams(n_bits=2, coef=np.array([0.5, -0.25, 0.5, -0.5, 0.25]), intercept=0.1875, s_x=0.5, zp_x=0,
                     s_w=0.25, q_w=np.array([2, -1, 2, -2, 1], dtype=np.int64), q_b=0)
    return CorpusQuant(qp, 2, 0.5), Q.QuantizedLinearParams.from_json(qp.to_dict())


@pytest.mark.parametrize("seeded", [False, True], ids=["full", "seeded"])
def test_two_rotations_end_to_end_toy(need_gpu, seeded):
    """An evaluation-only PrivateServer: generation 0 loads 20 documents;
    rotate, rekey, append 3; rotate(bridge_from=[g0, g1]), rekey, append 17.
    search_resident with Q = 3 and per-query thresholds decrypts, under the
    newest key, to quant_ref.corpus_* for all 40 documents."""
    from fheicp.corpus import EncryptedCorpus
    from fheicp.private import SEEDED_QUERY_MAGIC, PrivateClient, PrivateServer
    cq, oq = toy_model()
    rng = np.random.default_rng(77)
    docs = rng.uniform(-1.2, 0.7, (40, 5)).astype(np.float32)
    qs = rng.uniform(-1.2, 0.7, (3, 5)).astype(np.float32)
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, 2, q, docs) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    ts = [None, float(np.median(scores[1])), 0.5]
    want_below = np.stack([np.zeros(40, np.int64) if t is None else (scores[q] < t).astype(np.int64)
                           for q, t in enumerate(ts)])
    c0 = EncryptedCorpus(cq, scheme=TOY).compile(key_seed=99, device=0, noise_seed=6)
    g0 = PrivateClient(c0, count=TOY.N, pack_seed=17, enc_seed=12, seeded=seeded, mask_seed=40)
    server = PrivateServer(g0.eval_keys(), cq, c0.P0, device=0, scheme=c0.scheme)
    assert server.load(g0.encrypt_docs(docs[:20])) == 20
    g1 = g0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20, enc_seed=13, mask_seed=41)
    assert g1.gadget == g0.gadget and [k for k, _ in g1.generations] == [g0.key_id, g1.key_id]
    server.rekey(g1.eval_keys())
    assert server.append(g1.encrypt_docs(docs[20:23])) == 23
    g2 = g1.rotate(key_seed=9, pack_seed=21, bridge_seed=22, noise_seed=23, enc_seed=14, mask_seed=42,
                   bridge_from=[g0, g1])
    keys2 = g2.eval_keys()
    assert [str(x) for x in keys2["bridge_from"]] == [g0.key_id, g1.key_id] and "bridge_key" not in keys2
    assert keys2["bridge_keys"].shape[0] == 2 and tuple(keys2["bridge_gadget"]) == g2.bridge_gadget
    server.rekey(keys2)
    assert server.append(g2.encrypt_docs(docs[23:])) == 40
    assert server.generations == [(g0.key_id, 20), (g1.key_id, 23), (g2.key_id, 40)]
    assert server.old_generations == [(g0.key_id, 20), (g1.key_id, 23)]
    assert server.engine.bridge_slots() == [0, 1]
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):            # evaluation keys only
        server.engine.decrypt(server.engine.empty_big(1))
    bundle = g2.encrypt_queries_gens(qs)
    assert list(bundle) == [g0.key_id, g1.key_id, g2.key_id] and all(len(v) == 3 for v in bundle.values())
    assert all((int(p[0]) == SEEDED_QUERY_MAGIC) == seeded for v in bundle.values() for p in v)
    replies = server.search_resident(bundle, ts)
    assert len(replies) == 1
    acc, below = g2.decrypt_replies(replies)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(below.cpu().numpy(), want_below)
    for part in (slice(0, 20), slice(23, 40)):                         # bits on both sides in the large generations
        assert 0 < want_below[1, part].sum() < want_below[1, part].size
    if GROUPED:
        assert server.engine.kernel_name("linear_ggsws").startswith("k_extprod_queries_mfma_grp<")
    # a bundle with generations 0 and 1 swapped does not decode on their documents
    swapped = {g0.key_id: bundle[g1.key_id], g1.key_id: bundle[g0.key_id], g2.key_id: bundle[g2.key_id]}
    acc_s, _ = g2.decrypt_replies(server.search_resident(swapped, ts))
    acc_s = acc_s.cpu().numpy()
    np.testing.assert_array_equal(acc_s[:, 23:], ref[:, 23:])
    assert not np.array_equal(acc_s[:, :20], ref[:, :20]) and not np.array_equal(acc_s[:, 20:23], ref[:, 20:23])
    # generation 0's key holder cannot open the reply
    a0, _ = g0.decrypt_replies(replies)
    assert not np.array_equal(a0.cpu().numpy(), ref)
    # a bundle that lacks a resident generation is refused by its fingerprint
    with pytest.raises(ValueError, match=f"documents under key {g1.key_id} are resident"):
        server.search_resident({k: v for k, v in bundle.items() if k != g1.key_id}, ts)
    # a client that does not keep generation 0 says so
    with pytest.raises(ValueError, match="no client of generation"):
        g1.rotate(key_seed=11, bridge_seed=30).encrypt_queries_gens(qs, key_ids=[g0.key_id])
    server.engine.close()


# ------------------------------------------ noise at the real parameters --
def test_bridged_phase_noise_at_real_parameters(need_gpu):
    """P0 = 21, the 16-dim n_bits = 6 model, the query of tests/test_gpu_query.py,
    two generations of 64 documents: only the leveled step and the bridge run,
    and each generation's key holder reads phases. The statistic and the band
    are tests/test_gpu_extprod.py::test_extracted_phase_noise_at_real_parameters':
    the RMS phase error of 4096 rows against the model, sigma <= 1.1 sigma_model,
    the model now sqrt(extprod_var(||W||^2 of this query) + bridge_var): one
    more independent term. The 4096 bridged rows are 64 independent encryptions
    of the query against the old generation's 64 documents (the rounding of a
    document's words is shared by its 64 rows; the GGSW rows' noise and the
    bridge's digits are not)."""
    from fheicp.corpus import CorpusQuant
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    Xt, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(Xt, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    q, _ = Q.make_corpus(16, 256, seed=21)
    W = cq.weights(cq.quant(q))
    P0 = 21
    prm = params_for_bits(P0).with_msg_bits(P0)
    w2 = float(np.sum(W.astype(np.float64) ** 2))
    (beta, L), (bb, bL), _ = private_rotation_plan(prm, w2)
    old, new = Engine(prm, 0), Engine(prm, 0)
    old.keygen(6300)
    new.keygen(6301)
    s_old = old.export_key("s_big")
    new.keygen_bridge_key(s_old, bb, bL, seed=6302, slot=5)
    s_old[:] = 0
    rng = np.random.default_rng(21)
    Qn, Bg, D = 64, 64, 16
    dq = [rng.integers(cq.qmin, cq.qmax + 1, (Bg, D)) for _ in range(2)]
    items = []
    for g, eng in enumerate((old, new)):
        glwe = eng.encrypt_docs_glwe(dq[g], 31 + g, id0=0)
        ggsws = torch.cat([eng.encrypt_ggsw(W, beta, L, 33 + g, id0=1000 * i).reshape(-1) for i in range(Qn)])
        items.append((5 if g == 0 else -1, ggsws.contiguous(), new.pack_docs_glwe_queries(glwe, Bg, D, beta, L), Bg))
    rows = new.linear_ggsws_gens(items, beta, L, D, [0] * Qn)
    B = 2 * Bg
    idx = [torch.from_numpy(PG.gen_rows(Qn, [Bg, Bg], g)).to(new.device) for g in range(2)]

    def errors(eng, ct, g):
        ph = u64(eng.phase(ct.contiguous()))
        with np.errstate(over="ignore"):
            want = np.tile((dq[g] @ W).astype(U) << U(64 - P0), Qn)
            return (ph - want).view(np.int64).astype(np.float64)

    before = errors(old, rows[idx[0]], 0)                              # under the old key, before the bridge
    new.bridge_gens(rows, Qn, B, [Bg], [5])
    after = errors(new, rows[idx[0]], 0)                               # the same rows under the new key
    current = errors(new, rows[idx[1]], 1)
    ev, bv = extprod_var(prm, w2, beta, L), bridge_var(prm, bb, bL)
    model = math.sqrt(ev + bv)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    print(f"bridged rows ({beta},{L}) + bridge ({bb},{bL}), ||W||^2 = 2^{math.log2(w2):.2f}: sigma before "
          f"2^{math.log2(rms(before)):.2f}, after 2^{math.log2(rms(after)):.2f}, model 2^{math.log2(model):.2f} "
          f"(product 2^{math.log2(ev) / 2:.2f}, bridge 2^{math.log2(bv) / 2:.2f}), ratio {rms(after) / model:.3f}, "
          f"max |err| {np.abs(after).max() / model:.2f} model sigmas; current-generation rows ratio "
          f"{rms(current) / math.sqrt(ev):.3f}; bridge alone 2^{math.log2(rms(after - before)):.2f}")
    assert len(after) == 4096
    assert rms(after) <= 1.1 * model
    assert rms(current) <= 1.1 * math.sqrt(ev)
    assert np.abs(after).max() < 2.0 ** (63 - P0)                      # every bridged row still decodes
    old.close()
    new.close()
