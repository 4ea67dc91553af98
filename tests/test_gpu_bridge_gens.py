"""GPU: key rotation with several old generations resident.

fhe_bridge_gens_batch is word for word the numpy restatement
(tests/bridge_ref.py) applied segment by segment with each generation's key,
with and without the GEMM's K split, on random rows and on the bridge's edge
words at segment boundaries; at G = 1, slot 0 it is fhe_bridge_rows_batch and
the search entry is the bridged entry; the slot keygen, export, import and drop
entries; one kernel-level case on the P = 16 parameters; and an evaluation-only
CorpusServer with documents of three generations answers what the clear
restatement answers."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

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
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0)   # test_gpu_bridge.py's EDGE_ROWS patterns
BETA, LV = 4, 3
PERM8 = [3, 7, 0, 5, 1, 6, 2, 4]          # generation g -> bridge slot: not the identity
# (Q, B, ends): two generations; an empty one; 258 | 42 | 280 compact rows (three
# 128-blocks ending partial, a 16-row digit group crossed, a partial last block);
# nothing bridged; eight slots of one row each
CASES = [(1, 5, [2, 5]), (3, 7, [2, 2, 5]), (2, 300, [129, 150, 290]), (4, 16, [0, 0]),
         (1, 8, [1, 2, 3, 4, 5, 6, 7, 8])]


# the product library runs the grouped bridge; the per-generation loop exists as an A/B build only
GROUPED = Path(_lib.LIB_PATH).name == "libfheicp.so"


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def host_u64(t):
    return t.cpu().numpy().view(U)


def s_big_of(eng) -> np.ndarray:
    s = np.zeros(eng.big, U)
    eng._chk(eng._L.fhe_export_keys(eng._ctx, None, C.c_void_p(s.ctypes.data), None, None))
    return s


def segment_rows(Qn, B, ends):
    """Per generation, the rows {q B + b : ends[g-1] <= b < ends[g]} in compact order."""
    lo, out = 0, []
    for hi in ends:
        out.append(np.array([q * B + b for q in range(Qn) for b in range(lo, hi)], dtype=np.int64))
        lo = hi
    return out


def segmented_ref(ct, Qn, B, ends, keys, beta, lv, cols=None):
    """bridge_ref segment by segment with keys[g]; every other row unchanged."""
    want = np.array(ct, dtype=U, copy=True) if cols is None else np.array(ct[:, cols], dtype=U, copy=True)
    for idx, bk in zip(segment_rows(Qn, B, ends), keys):
        if idx.size:
            want[idx] = BR.bridge_ref(ct[idx], bk, beta, lv, cols=cols)
    return want


# ------------------------------------------------------ bit-exact on TOY --
@pytest.fixture(scope="module")
def toy8(need_gpu):
    """An evaluation-only TOY context with eight distinct numpy-made keys of
    uniform words, gadget (4, 3): keys[g] sits in slot PERM8[g]."""
    eng = Engine(TOY, 0)
    rng = np.random.default_rng(2024)
    big = TOY.k * TOY.N
    keys = [rng.integers(0, 2 ** 64, (big, LV, big + 1), dtype=U) for _ in range(8)]
    for g, bk in enumerate(keys):
        eng.import_bridge_key(BETA, LV, bk, slot=PERM8[g])
    assert eng.bridge_slots() == list(range(8))
    yield eng, keys
    eng.close()


def check_gens(eng, keys, ct, Qn, B, ends, expect_rows=None):
    """ct [Q B + 1, W] with a canary last; runs the entry in place and
    compares the whole buffer with the restatement."""
    G = len(ends)
    want = segmented_ref(ct, Qn, B, ends, keys[:G], BETA, LV)
    x = dev_u64(eng, ct)
    eng.profile(True)
    try:
        eng.bridge_gens(x, Qn, B, ends, PERM8[:G])
        prof = eng.profile_read("bridge")
    finally:
        eng.profile(False)
    rows = Qn * ends[-1]
    if expect_rows is not None:
        assert rows == expect_rows
    # one bracket for all generations; a -DFHEICP_GRP_BRIDGE=0 build (FHEICP_LIB) has one per non-empty generation
    brackets = 1 if GROUPED else len({e for e in ends if e})
    assert (prof["launches"], prof["items"]) == ((brackets, rows) if rows else (0, 0))
    got = host_u64(x)
    np.testing.assert_array_equal(got, want)
    bridged = np.concatenate(segment_rows(Qn, B, ends)) if rows else np.zeros(0, np.int64)
    assert len(bridged) == rows and (rows == 0 or not np.array_equal(got[bridged], ct[bridged]))
    untouched = np.setdiff1d(np.arange(Qn * B + 1), bridged)
    assert (got[untouched] == U(CANARY)).all()


def canaried(rng, eng, Qn, B, ends):
    """Random words on the old generations' rows, the canary word on every
    current-key row and on the row after the buffer."""
    ct = np.full((Qn * B + 1, eng.W), CANARY, dtype=U)
    for idx in segment_rows(Qn, B, ends):
        if idx.size:
            ct[idx] = rng.integers(0, 2 ** 64, (idx.size, eng.W), dtype=U)
    return ct


@pytest.mark.parametrize("Qn,B,ends", CASES, ids=[f"q{q}b{b}g{len(e)}" for q, b, e in CASES])
def test_bridge_gens_bit_exact_toy(toy8, Qn, B, ends):
    """The cases of up to 7 blocks (x 33 column blocks: room for a split) run
    the K-split GEMM, atomics into zeroed compact rows; the eight one-row
    generations are 8 blocks, 264 tiles, and run it unsplit."""
    eng, keys = toy8
    rng = np.random.default_rng(Qn * 1000 + B)
    check_gens(eng, keys, canaried(rng, eng, Qn, B, ends), Qn, B, ends)
    if (Qn, B) == (2, 300):
        assert eng.kernel_name("bridge") == ("k_keyswitch_mfma_grp<8, 1>" if GROUPED else "k_keyswitch_mfma<8, 1>")


def test_bridge_gens_unsplit_gemm_bit_exact_toy(toy8):
    """B = 300, ends [129, 150, 290] with the GEMM unsplit, forced as
    test_bridge_unsplit_gemm_bit_exact_toy forces it: by row count. The split
    rule leaves S = 1 above 256 tiles of (128-row block) x (column block); TOY
    has 33 column blocks, so 8 blocks are needed. At Q = 2 these ends make
    3 + 1 + 3 = 7 blocks (231 tiles, S = 2: the parametrised case above); at
    Q = 3 the segments hold 387, 63 and 420 rows, 4 + 1 + 4 = 9 blocks, 297
    tiles, and the GEMM stores instead of adding. Every segment still ends
    partial."""
    eng, keys = toy8
    Qn, B, ends = 3, 300, [129, 150, 290]
    blocks = sum(-(-Qn * n // 128) for n in (129, 21, 140))
    assert blocks * 33 > 256 >= 7 * 33
    rng = np.random.default_rng(77)
    check_gens(eng, keys, canaried(rng, eng, Qn, B, ends), Qn, B, ends, expect_rows=870)


def test_bridge_gens_edge_rows_at_segment_boundaries(toy8):
    """The edge words (digits at both ends of their range, ties with both
    coins) on the first and last document of every generation, for both
    queries."""
    eng, keys = toy8
    Qn, B, ends = 2, 300, [129, 150, 290]
    rng = np.random.default_rng(99)
    ct = canaried(rng, eng, Qn, B, ends)
    for q in range(Qn):
        for i, b in enumerate((0, 128, 129, 149, 150, 289, 1, 127)):
            ct[q * B + b, :] = U(EDGE_WORDS[(i + q) % 4])
    check_gens(eng, keys, ct, Qn, B, ends)


@pytest.mark.parametrize("Qn,B,B_old", [(3, 7, 2), (2, 20, 17), (1, 5, 5)])
def test_one_generation_in_slot_0_is_the_row_map_bridge(need_gpu, Qn, B, B_old):
    """G = 1, h_slots = {0}: fhe_bridge_rows_batch word for word."""
    eng = Engine(TOY, 0)
    rng = np.random.default_rng(B)
    big = TOY.k * TOY.N
    eng.import_bridge_key(BETA, LV, rng.integers(0, 2 ** 64, (big, LV, big + 1), dtype=U))
    ct = rng.integers(0, 2 ** 64, (Qn * B + 1, eng.W), dtype=U)
    a, b = dev_u64(eng, ct), dev_u64(eng, ct)
    eng.bridge_rows(a, Qn, B, B_old)
    eng.bridge_gens(b, Qn, B, [B_old], [0])
    assert torch.equal(a, b) and not np.array_equal(host_u64(a), ct)
    np.testing.assert_array_equal(host_u64(b)[Qn * B], ct[Qn * B])
    eng.close()


def test_context_entry_is_the_group_entry_of_one_tenant(toy8):
    """fhe_bridge_gens_batch on a context and fhe_bridge_group_gens_batch on a
    group of that one context (its rows start at row 0 of the padded buffer):
    the same eight keys, (Q, B, ends) = (2, 300, [129, 150, 290]); equal words
    on all Q B rows, the row after them untouched. The context has evaluation
    keys of its own: a group admits no other."""
    from fheicp.engine import EngineGroup
    _, keys = toy8
    eng = Engine(TOY, 0)
    eng.keygen(311)
    for g, bk in enumerate(keys):
        eng.import_bridge_key(BETA, LV, bk, slot=PERM8[g])
    grp = EngineGroup([eng])
    try:
        Qn, B, ends = 2, 300, [129, 150, 290]
        ct = canaried(np.random.default_rng(23), eng, Qn, B, ends)
        a, b = dev_u64(eng, ct), dev_u64(eng, ct)
        eng.bridge_gens(a, Qn, B, ends, PERM8[:3])
        grp.bridge_gens(b, [(Qn, B, ends, PERM8[:3])])
        ga, gb = host_u64(a), host_u64(b)
        np.testing.assert_array_equal(ga[:Qn * B], gb[:Qn * B])
        bridged = np.concatenate(segment_rows(Qn, B, ends))
        assert not np.array_equal(ga[bridged], ct[bridged])             # and the bridge did something
        assert (ga[Qn * B] == U(CANARY)).all() and (gb[Qn * B] == U(CANARY)).all()
    finally:
        grp.close()
        eng.close()


# ------------------------------------------------------------- slot keys --
def test_slot_keygen_export_import_drop(need_gpu):
    eng = Engine(TOY, 0)
    eng.keygen(77)
    rng = np.random.default_rng(3)
    s_old = rng.integers(0, 2, eng.big, dtype=U)
    eng.keygen_bridge_key(s_old, BETA, LV, seed=5)
    bk0 = eng.export_bridge_key()
    # the courtesy check: a live slot was generated with this key
    with pytest.raises(_lib.FheError, match="FHE_E_ARG.*key reuse.*slot 0"):
        eng.keygen_bridge_key(s_old, BETA, LV, seed=5, slot=3)
    assert eng.bridge_slots() == [0]
    eng.keygen_bridge_key(s_old, BETA, LV, seed=6)                      # slot 0 moves to another key
    assert (eng.export_bridge_key() != bk0).mean() > 0.99
    eng.keygen_bridge_key(s_old, BETA, LV, seed=5, slot=2)              # the same inputs in slot 2: the same key
    np.testing.assert_array_equal(eng.export_bridge_key(2), bk0)
    assert eng.bridge_slots() == [0, 2] and eng.bridge_gadget_of(2) == (BETA, LV)
    # the rows decrypt to their messages under the context's secret
    ph = BR.lwe_phase(bk0.reshape(-1, eng.big + 1), s_big_of(eng)).reshape(eng.big, LV)
    with np.errstate(over="ignore"):
        for l in range(LV):
            ph[:, l] -= s_old << U(64 - BETA * (l + 1))
    assert np.abs(ph.astype(np.int64)).max() <= 1 << TOY.glwe_noise_bits
    # export / import round trip into another slot of a context without any other key
    S = Engine(TOY, 0)
    S.import_bridge_key(BETA, LV, bk0, slot=5)
    np.testing.assert_array_equal(S.export_bridge_key(5), bk0)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no bridge key"):
        S.export_bridge_key()                                           # slot 0 is still empty
    # the seeded form: generated in slot 1, shipped as bodies, imported to the same words
    mk = np.arange(8, dtype=np.uint32) + 11
    eng.keygen_bridge_key(s_old, BETA, LV, seed=8, mask_key=mk, slot=1)
    full1 = eng.export_bridge_key(1)
    got_mk, body = eng.export_bridge_key_seeded(1)
    np.testing.assert_array_equal(got_mk, mk)
    assert body.size == eng.big * LV
    S.import_bridge_key_seeded(BETA, LV, got_mk, body, slot=4)
    np.testing.assert_array_equal(S.export_bridge_key(4), full1)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*seeded"):
        eng.export_bridge_key_seeded(2)                                 # slot 2 was not generated seeded
    # one mask key serves one generated key, whatever the slot
    with pytest.raises(_lib.FheError, match="FHE_E_ARG.*mask key reuse"):
        eng.keygen_bridge_key(s_old, BETA, LV, seed=9, mask_key=mk, slot=6)
    # drop, then use: FHE_E_STATE naming the slot; a slot without rows needs no key
    ct = dev_u64(S, rng.integers(0, 2 ** 64, (8, S.W), dtype=U))
    S.bridge_gens(ct.clone(), 2, 4, [1, 3], [5, 4])
    S.drop_bridge_key(4)
    assert S.bridge_slots() == [5]
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no bridge key in slot 4"):
        S.bridge_gens(ct.clone(), 2, 4, [1, 3], [5, 4])
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: no bridge key in slot 4"):
        S._chk(S._L.fhe_export_bridge_key_slot(S._ctx, 4, C.c_void_p(np.zeros(bk0.size, U).ctypes.data)))
    before = ct.clone()
    S.bridge_gens(ct, 2, 4, [1, 1], [5, 4])                             # generation 1 is empty
    assert not torch.equal(ct, before)
    S.drop_bridge_key(4)                                                # an empty slot: nothing to do
    # differing gadgets
    big = TOY.k * TOY.N
    S.import_bridge_key(7, 6, rng.integers(0, 2 ** 64, (big, 6, big + 1), dtype=U), slot=6)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE: bridge gadgets differ"):
        S.bridge_gens(ct, 2, 4, [1, 3], [5, 6])
    S.bridge_gens(ct, 2, 4, [1, 1], [5, 6])                             # ... unless the other slot has no rows
    S.close()
    eng.close()


# ----------------------------------------- real parameters, sampled columns --
def test_bridge_gens_sampled_columns_p16(need_gpu):
    """Two key holders on the P = 16 parameters (test_gpu_bridge.py's p16_pair
    construction): B holds a bridge from A's key in slot 0 and one from a
    third key in slot 1; (1, 300, [129, 300]), so both segments end in a
    partial block, at kN + 1 columns and the planned gadget's K depth.
    Sixty-four sampled columns plus the body against the restatement on the
    exported keys' columns, and A's messages decrypt under B."""
    p = params_for_bits(16)
    beta, lv = bridge_plan(p, 0.0)
    A, B_ = Engine(p, 0), Engine(p, 0)
    A.keygen(501)
    B_.keygen(502)
    big = p.k * p.N
    rng = np.random.default_rng(16)
    B_.keygen_bridge_key(s_big_of(A), beta, lv, seed=9)
    B_.keygen_bridge_key(rng.integers(0, 2, big, dtype=U), beta, lv, seed=10, slot=1)
    keys = [B_.export_bridge_key(s).reshape(big, lv, big + 1) for s in (0, 1)]
    Qn, Bd, ends = 1, 300, [129, 300]
    P = p.msg_bits
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), 129)
    ct = rng.integers(0, 2 ** 64, (301, big + 1), dtype=U)
    ct[:129] = host_u64(A.encrypt(msgs, seed=12, id0=3)).reshape(129, big + 1)
    ct[200, :] = U(0x8080808080808080)
    ct[300] = U(CANARY)
    x = dev_u64(B_, ct)
    B_.bridge_gens(x, Qn, Bd, ends, [0, 1])
    got = host_u64(x)
    cols = np.unique(np.concatenate([rng.choice(np.arange(1, big - 1), 62, replace=False), [0, big - 1, big]]))
    assert len(cols) == 65 and cols[-1] == big       # 64 mask columns, both ends among them, and the body
    np.testing.assert_array_equal(got[:, cols], segmented_ref(ct, Qn, Bd, ends, keys, beta, lv, cols=cols))
    assert (got[300] == U(CANARY)).all()
    np.testing.assert_array_equal(B_.decrypt(x[:129]).cpu().numpy(), msgs)
    A.close()
    B_.close()


# ------------------------------------------------------------ end to end --
def toy_model():
    """test_gpu_bridge.py's hand-made 5-feature model: q_w in {-1, 0, 1}, 2-bit
    document and query values, P0 = 7."""
    from fheicp.corpus import CorpusQuant
    from fheicp.model import QuantParams
    qp = QuantParams(n_bits=2, coef=np.array([1.0, -1.0, 1.0, 0.0, 1.0]), intercept=1.0, s_x=1.0, zp_x=0, s_w=1.0,
                     q_w=np.array([1, -1, 1, 0, 1], dtype=np.int64), q_b=1)
    cq = CorpusQuant(qp, 2, 1.0)
    return cq, Q.QuantizedLinearParams.from_json(qp.to_dict())


def rotation_scenario(seeded: bool = False):
    """Clients of generations 0 -> 1 -> 2, the last with direct bridges from
    both earlier ones; an evaluation-only server that lived through both
    rotations with 12 + 5 + 3 documents; two queries. Every seed is fixed, so
    two runs give the same words. seeded: the evaluation keys and the bridge
    keys travel in the seeded form."""
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusServer
    cq, oq = toy_model()
    c0 = EncryptedCorpus(cq, TOY).compile(key_seed=5, device=0, noise_seed=6,
                                          mask_key=np.arange(8, dtype=np.uint32) + 41,   # given: its default is random
                                          seeded_keys=seeded, key_mask_seed=700 if seeded else None)
    client0 = CorpusClient(c0, pack_seed=17)
    rng = np.random.default_rng(8)
    docs = rng.integers(-2, 2, (20, 5)).astype(np.float32)
    queries = np.array([[1, -2, 1, 1, -1], [1, 1, 1, 1, 1]], np.float32)
    client1 = client0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
    client2 = client1.rotate(key_seed=9, pack_seed=21, bridge_seed=22, noise_seed=23, bridge_from=[client0, client1])
    server = CorpusServer(client0.eval_keys(), cq, c0.P0, c0.mask_key, scheme=c0.scheme)
    # generation 0's stream ids are given (its default ids are random); the rotated clients' continue after them
    server.load(*client0.encrypt_docs(docs[:12], id0=np.arange(12, dtype=U) * U(5) + U(1000)))
    server.rekey(client1.eval_keys())
    server.append(*client1.encrypt_docs(docs[12:17]))
    keys2 = client2.eval_keys()
    server.rekey(keys2)
    server.append(*client2.encrypt_docs(docs[17:]))
    scores = np.stack([Q.corpus_accumulate(oq, cq.s_e, cq.n_e, q, docs) for q in queries]).astype(np.float64)
    ts = [float(np.median(scores[0])), float(np.median(scores[1])) + 0.5]
    return {"cq": cq, "oq": oq, "clients": (client0, client1, client2), "server": server, "docs": docs,
            "queries": queries, "ts": ts, "keys2": keys2, "scores": scores}


def dump_replies(path):
    """The scenario's replies -> an .npz (the child process of the A/B comparison)."""
    f = rotation_scenario()
    np.savez(path, *f["server"].search_many(f["queries"], f["ts"]))


def restated(f):
    ref = np.stack([Q.corpus_accumulate(f["oq"], f["cq"].s_e, f["cq"].n_e, q, f["docs"]) for q in f["queries"]])
    sc = np.float64(Q.corpus_out_scale(f["oq"], f["cq"].s_e)) * ref.astype(np.float64)
    return ref, np.stack([(sc[i] < t).astype(np.int64) for i, t in enumerate(f["ts"])])


def test_three_generations_seeded_keys_toy(need_gpu):
    """The same store with seeded keys: the bridges travel as bridge_key_bodies
    [G, kN L] and bridge_mask_keys [G, 8], each under a mask key of its own,
    and the rekeyed server answers what the restatement answers."""
    f = rotation_scenario(seeded=True)
    client0, client1, client2 = f["clients"]
    server, keys2 = f["server"], f["keys2"]
    eng = server.engine
    b, L = client2.bridge_gadget
    assert "bridge_keys" not in keys2 and "bridge_key_body" not in keys2 and "bsk_body" in keys2
    assert keys2["bridge_key_bodies"].shape == (2, eng.big * L) and keys2["bridge_mask_keys"].shape == (2, 8)
    masks = {bytes(np.asarray(keys2[k], np.uint32).tobytes()) for k in ("eval_mask_key", "pack_mask_key")}
    masks |= {bytes(np.asarray(m, np.uint32).tobytes()) for m in keys2["bridge_mask_keys"]}
    assert len(masks) == 4                                              # one mask key serves one generated key
    assert [str(x) for x in keys2["bridge_from"]] == [client0.key_id, client1.key_id]
    assert eng.bridge_slots() == [0, 1]
    assert server.generations == [(client0.key_id, 12), (client1.key_id, 17), (client2.key_id, 20)]
    # the imported slots hold the words the key holder's slots hold
    for slot in (0, 1):
        np.testing.assert_array_equal(eng.export_bridge_key(slot), client2.corpus.engine.export_bridge_key(slot))
    acc, below = client2.decrypt_replies(server.search_many(f["queries"], f["ts"]))
    ref, want_below = restated(f)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(below.cpu().numpy(), want_below)


VARIANT = Path(_lib.LIB_PATH).with_name("libfheicp_grpbridge0.so")


def test_three_generations_end_to_end_toy(need_gpu, tmp_path):
    f = rotation_scenario()
    cq, oq, docs, queries, ts = f["cq"], f["oq"], f["docs"], f["queries"], f["ts"]
    client0, client1, client2 = f["clients"]
    server, keys2 = f["server"], f["keys2"]
    assert [str(x) for x in keys2["bridge_from"]] == [client0.key_id, client1.key_id]
    assert keys2["bridge_keys"].shape == (2, server.engine.bridge_key_words(*client2.bridge_gadget))
    assert "bridge_key" not in keys2 and tuple(keys2["bridge_gadget"]) == client2.bridge_gadget
    assert not np.array_equal(keys2["bridge_keys"][0], keys2["bridge_keys"][1])
    assert server.generations == [(client0.key_id, 12), (client1.key_id, 17), (client2.key_id, 20)]
    assert server.engine.bridge_slots() == [0, 1]
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):            # evaluation keys only
        server.engine.decrypt(server.engine.empty_big(1))
    replies = server.search_many(queries, ts)
    acc, below = client2.decrypt_replies(replies)
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, cq.n_e, q, docs) for q in queries])
    sc = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    want_below = np.stack([(sc[i] < t).astype(np.int64) for i, t in enumerate(ts)])
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(below.cpu().numpy(), want_below)
    for part in (slice(0, 12), slice(12, 17), slice(17, 20)):           # every generation has bits on both sides
        assert 0 < want_below[:, part].sum() < want_below[:, part].size
    # the generation-1 key holder cannot open the new replies
    a1, _ = client1.decrypt_replies(replies)
    assert not np.array_equal(a1.cpu().numpy(), ref)
    # the search entry at G = 0 and G = 1, slot 0 is the bridged entry word for word
    eng = server.engine
    Wr, cst, Ts, P = server._plan.plan_many(queries, ts)
    eng.set_msg_bits(P)
    Wd = eng.to_dev(Wr)
    for b_old in (0, 12):
        ga, gb = eng.search_seeded_queries(server.body, server.ids, server.mask_key, Wd, cst, Ts, server.bit_levels,
                                           b_old=b_old)
        ga2, gb2 = eng.search_seeded_queries_gens(server.body, server.ids, server.mask_key, Wd, cst, Ts,
                                                  server.bit_levels, gen_ends=[12] if b_old else [],
                                                  gen_slots=[0] if b_old else [])
        torch.cuda.synchronize()
        assert torch.equal(ga, ga2) and torch.equal(gb, gb2), b_old
    if b_old:                                                           # and the bridge did something
        ga0, _ = eng.search_seeded_queries(server.body, server.ids, server.mask_key, Wd, cst, Ts, server.bit_levels)
        assert not torch.equal(ga, ga0)
    # the eval-keys file round trip rekeys another server the same way
    from fheicp.query import load_eval_keys, save_eval_keys
    save_eval_keys(str(tmp_path / "k2.npz"), keys2)
    got = load_eval_keys(str(tmp_path / "k2.npz"))
    np.testing.assert_array_equal(got["bridge_keys"], keys2["bridge_keys"])
    # a per-generation-loop build of the library, where one was built: the same words
    if VARIANT.exists() and Path(_lib.LIB_PATH) != VARIANT:
        out = tmp_path / "loop.npz"
        env = dict(os.environ, FHEICP_LIB=str(VARIANT))
        code = f"import sys; sys.path[:0] = {[str(Path(__file__).parent)] + sys.path!r}; " \
               f"import test_gpu_bridge_gens as T; T.dump_replies({str(out)!r})"
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
        with np.load(out) as z:
            loop = [z[k] for k in z.files]
        assert len(loop) == len(replies)
        for a, b in zip(replies, loop):
            np.testing.assert_array_equal(a, b)
