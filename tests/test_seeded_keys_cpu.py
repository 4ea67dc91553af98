"""CPU: seeded evaluation keys, the parts that need no GPU:
the numpy restatement of the two expansions (tests/seeded_keys_ref.py) pinned
to the oracle's key generation, the ABI's size functions, how the Python side
tells the two dict forms apart and what it refuses, the new entry points on a
host-only context, and the .npz round trip of a seeded dict."""
import ctypes as C
import re
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import seeded_keys_ref as S

from fheicp import _lib
from fheicp.params import TOY, params_for_bits

REPO = Path(__file__).resolve().parents[1]
U = np.uint64
# TOY (n = 64) and TOY with an odd n and one multi-bit gadget: an odd pair count
# (31 pairs), a partly used last ChaCha block (61 = 7 * 8 + 5) and rows of 62
# words, 496 bytes: 8-byte aligned and no more
TOY_MB = replace(TOY, n=61, pbs_base_log=12, pbs_level=3, pbs_fast_base_log=8, pbs_fast_level=2, pbs_fast_group=2)
DEFAULTS = params_for_bits(16)
SIZES = ("fhe_bsk_body_words", "fhe_ksk_body_words", "fhe_fast_bsk_body_words", "fhe_pack_key_body_words",
         "fhe_bridge_key_body_words")
NEW_INT = ("fhe_keygen_seeded", "fhe_keygen_pack_key_seeded", "fhe_keygen_bridge_key_seeded",
           "fhe_export_eval_keys_seeded", "fhe_export_pack_key_seeded", "fhe_export_bridge_key_seeded",
           "fhe_import_eval_keys_seeded", "fhe_import_pack_key_seeded", "fhe_import_bridge_key_seeded")


# --------------------------------------------------------------- restatement --
def check_bsk_forms(key, msgs, s_big, mask_key, tag, prm, L, beta):
    """One bootstrapping key of the oracle against the restatement. Its rows
    with c = k, and with c < k where the message is 0, are their bodies'
    expansion word for word. A row (i, c < k, l) with message 1 is not: word cN
    of its MASK is the stream word plus g_l = 2^(64 - l beta), so the one-key
    form has no body-only form and a public mask key would give the message
    away. The seeded keygen's form (messages_to_body: mask = stream, body - g_l
    S_c) is the expansion of its bodies word for word."""
    N, k = prm.N, prm.k
    key = np.asarray(key, U)
    plain = S.expand_glwe_rows(S.glwe_row_bodies(key, N, k), mask_key, tag, N, k)
    diff = (key - plain).reshape(len(msgs), k + 1, L, k + 1, N)
    want = np.zeros_like(diff)
    for l in range(1, L + 1):
        for c in range(k):
            want[:, c, l - 1, c, 0] = np.asarray(msgs, U) << U(64 - l * beta)
    np.testing.assert_array_equal(diff, want)
    assert np.count_nonzero(want) == k * L * int(np.sum(msgs)) > 0
    seeded = S.messages_to_body(key, msgs, s_big, N, k, L, beta)
    body = S.glwe_row_bodies(seeded, N, k)
    np.testing.assert_array_equal(S.expand_glwe_rows(body, mask_key, tag, N, k), seeded)
    # both forms are the same encryptions: equal rows with c = k, equal phases b - sum_c a_c S_c
    # on the others (checked on the first GGSW whose message is 1)
    i = int(np.flatnonzero(msgs)[0])
    a = key.reshape(len(msgs), k + 1, L, k + 1, N)[i]
    b = seeded.reshape(len(msgs), k + 1, L, k + 1, N)[i]
    np.testing.assert_array_equal(a[k], b[k])
    Sb = np.asarray(s_big, U).reshape(k, N)
    from oracle import tfhe_ref
    for c in range(k):
        for x in (a, b):
            ph = x[c, 0, k].copy()
            for j in range(k):
                ph -= tfhe_ref.negacyclic_mul(x[c, 0, j], Sb[j])
            err = (ph + (U(1) << U(64 - beta)) * Sb[c]).astype(np.int64)          # e - g S_c + g S_c
            assert np.abs(err).max() <= 2 ** prm.glwe_noise_bits
    return body


@pytest.mark.parametrize("prm", [TOY, TOY_MB], ids=["n64", "n61_multibit"])
def test_restatement_expands_the_oracles_keys(oracle_lib, prm):
    """The oracle's ksk, stripped to its bodies and expanded again under the
    keygen seed's ChaCha key, word for word; its bsk and multi-bit gadget key
    likewise once their messages sit in the bodies (check_bsk_forms)."""
    seed = 4321
    ref = oracle_lib.RefTFHE(prm.as_dict(), seed)
    key = oracle_lib.key_from_seed(seed)
    N, k, n = prm.N, prm.k, prm.n
    body = check_bsk_forms(ref.bsk, ref.s_small, ref.s_big, key, S.TAG_BSK_MASK, prm, prm.pbs_level, prm.pbs_base_log)
    assert body.shape == (n * (k + 1) * prm.pbs_level, N)
    kb = S.lwe_row_bodies(ref.ksk, n + 1)
    assert kb.shape == (k * N * prm.ks_level,)
    np.testing.assert_array_equal(S.expand_lwe_rows(kb, key, S.TAG_KSK_MASK, n + 1), ref.ksk)
    assert (1 in ref.keys) == (prm is TOY_MB)
    if prm is TOY_MB:
        assert S.gadget_tag(prm, 1) == S.TAG_MB_MASK[1]
        msgs = S.mb_messages(ref.s_small)
        assert msgs.size == 3 * 31                                          # three GGSWs per pair, 31 pairs
        gb = check_bsk_forms(ref.keys[1], msgs, ref.s_big, key, S.TAG_MB_MASK[1], prm, prm.pbs_fast_level,
                             prm.pbs_fast_base_log)
        assert gb.shape == (3 * 31 * (k + 1) * prm.pbs_fast_level, N)
        # under the classic key's tag the masks differ: the tag is part of the address
        assert not np.array_equal(S.expand_glwe_rows(gb[:2], key, S.TAG_GADGET_MASK[1], N, k)[:N],
                                  ref.keys[1][:N])
    # the dict form, as Engine.export_eval_keys(seeded=True) lays it out
    d = {"eval_mask_key": key, "bsk_body": body.reshape(-1), "ksk_body": kb}
    if prm is TOY_MB:
        d["gadget_bsk1_body"] = gb.reshape(-1)
    full = S.expand_eval_keys(d, prm)
    np.testing.assert_array_equal(full["bsk"], S.messages_to_body(ref.bsk, ref.s_small, ref.s_big, N, k,
                                                                  prm.pbs_level, prm.pbs_base_log))
    np.testing.assert_array_equal(full["ksk"], ref.ksk)
    # every ksk row decrypts under the oracle's secrets to its message and a TUniform noise
    ph = S.lwe_row_phases(ref.ksk, n + 1, ref.s_small).reshape(k * N, prm.ks_level)
    msg = ref.s_big[:, None] << (U(64) - U(prm.ks_base_log) * np.arange(1, prm.ks_level + 1, dtype=U))[None, :]
    err = (ph - msg).astype(np.int64)
    assert np.abs(err).max() <= 2 ** prm.lwe_noise_bits


# --------------------------------------------------------------------- sizes --
def test_size_functions():
    L = _lib.lib()
    for p in (TOY, TOY_MB, DEFAULTS, params_for_bits(21)):
        P = _lib.params_struct(p.as_dict())
        big = p.k * p.N
        assert L.fhe_bsk_body_words(C.byref(P)) == p.n * (p.k + 1) * p.pbs_level * p.N
        assert L.fhe_bsk_body_words(C.byref(P)) * (p.k + 1) == L.fhe_bsk_words(C.byref(P))
        assert L.fhe_ksk_body_words(C.byref(P)) == big * p.ks_level
        assert L.fhe_ksk_body_words(C.byref(P)) * (p.n + 1) == L.fhe_ksk_words(C.byref(P))
        for g in range(0, 7):
            full = L.fhe_fast_bsk_words(C.byref(P), g)
            assert L.fhe_fast_bsk_body_words(C.byref(P), g) * (p.k + 1) == full, g
        for beta in range(0, 9):
            for lv in range(0, 10):
                pk, bk = L.fhe_pack_key_words(C.byref(P), beta, lv), L.fhe_bridge_key_words(C.byref(P), beta, lv)
                pb = L.fhe_pack_key_body_words(C.byref(P), beta, lv)
                bb = L.fhe_bridge_key_body_words(C.byref(P), beta, lv)
                if pk == 0:                                         # a rejected gadget
                    assert pb == 0 and bb == 0 and bk == 0, (beta, lv)
                else:
                    assert pb == big * lv * p.N and pb * (p.k + 1) == pk, (beta, lv)
                    assert bb == big * lv and bb * (big + 1) == bk, (beta, lv)
    assert L.fhe_bsk_body_words(None) == 0 and L.fhe_ksk_body_words(None) == 0
    assert L.fhe_fast_bsk_body_words(None, 1) == 0
    assert L.fhe_pack_key_body_words(None, 4, 3) == 0 and L.fhe_bridge_key_body_words(None, 4, 3) == 0
    # the default parameters: n = 887, k = 2, N = 1024, main gadget (15, 2), key switch (3, 5)
    p = DEFAULTS
    assert (p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level) == (887, 2, 1024, 15, 2, 3, 5)
    P = _lib.params_struct(p.as_dict())
    assert L.fhe_bsk_words(C.byref(P)) == 16_349_184 and L.fhe_bsk_body_words(C.byref(P)) == 5_449_728
    assert L.fhe_ksk_words(C.byref(P)) == 9_093_120 and L.fhe_ksk_body_words(C.byref(P)) == 10_240
    assert p.pbs_fast_group == 2                                    # a multi-bit key: 3 * ceil(n / 2) GGSWs
    assert L.fhe_fast_bsk_body_words(C.byref(P), 1) == 3 * 444 * 3 * p.pbs_fast_level * 1024
    # TOY: 64 * 3 * 2 rows of 256 body words; 512 * 4 rows of one
    T = _lib.params_struct(TOY.as_dict())
    assert L.fhe_bsk_body_words(C.byref(T)) == 98_304 and L.fhe_ksk_body_words(C.byref(T)) == 2_048
    assert L.fhe_fast_bsk_body_words(C.byref(T), 1) == 0            # TOY has no fast gadget
    assert L.fhe_pack_key_body_words(C.byref(T), 4, 3) == 512 * 3 * 256
    assert L.fhe_bridge_key_body_words(C.byref(T), 4, 3) == 512 * 3


def test_new_exports_present_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fhe_icp.h").read_text(), flags=re.S)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    integ = (REPO / "integration" / "fhe_gpu.py").read_text()
    L = _lib.lib()
    for name in NEW_INT + SIZES:
        ret = "int" if name in NEW_INT else "size_t"
        m = re.search(r"^" + ret + " " + name + r"\((.*?)\);", hdr, flags=re.S | re.M)
        assert m, name
        assert len(bound[name]) == m.group(1).count(",") + 1, name    # one ctypes argument per C parameter
        assert hasattr(L, name)
    assert hdr.index("fhe_search_ggsws_seeded_batch") < min(hdr.index(n) for n in NEW_INT + SIZES)     # appended
    for name in SIZES + ("fhe_import_eval_keys_seeded", "fhe_import_pack_key_seeded", "fhe_import_bridge_key_seeded"):
        assert f'"{name}"' in integ, name
    from fheicp.engine import Engine
    for meth in ("export_pack_key_seeded", "import_pack_key_seeded", "export_bridge_key_seeded",
                 "import_bridge_key_seeded"):
        assert callable(getattr(Engine, meth))


# ---------------------------------------------------------------- dict forms --
def seeded_dict(p, pack=(4, 3), bridge=(7, 7)):
    L = _lib.lib()
    P = _lib.params_struct(p.as_dict())
    d = {"eval_mask_key": np.arange(8, dtype=np.uint32),
         "bsk_body": np.zeros(L.fhe_bsk_body_words(C.byref(P)), U),
         "ksk_body": np.zeros(L.fhe_ksk_body_words(C.byref(P)), U)}
    if p.pbs_fast_level:
        d["gadget_bsk1_body"] = np.zeros(L.fhe_fast_bsk_body_words(C.byref(P), 1), U)
    if pack:
        d.update(pack_key_body=np.zeros(L.fhe_pack_key_body_words(C.byref(P), *pack), U),
                 pack_mask_key=np.arange(8, 16, dtype=np.uint32), pack_gadget=np.array(pack, np.int64))
    if bridge:
        d.update(bridge_key_body=np.zeros(L.fhe_bridge_key_body_words(C.byref(P), *bridge), U),
                 bridge_mask_key=np.arange(16, 24, dtype=np.uint32), bridge_gadget=np.array(bridge, np.int64))
    return d


def test_dict_form_dispatch_and_refusals():
    from fheicp.engine import eval_keys_seeded, seeded_eval_key_sizes
    d = seeded_dict(TOY_MB)
    assert eval_keys_seeded(d) is True
    assert eval_keys_seeded({"bsk": np.zeros(1, U), "ksk": np.zeros(1, U), "pack_key": np.zeros(1, U)}) is False
    # the clients' extras change nothing
    assert eval_keys_seeded(dict(d, key_id=np.array(["ab"]), pack_bit_levels=np.array([2]),
                                 bridge_from=np.array(["cd"]))) is True
    for full in ("bsk", "ksk", "gadget_bsk1", "pack_key", "bridge_key"):
        with pytest.raises(ValueError, match="mix the seeded and the full form.*" + full):
            eval_keys_seeded(dict(d, **{full: np.zeros(4, U)}))
    with pytest.raises(ValueError, match="mix the seeded and the full form"):
        eval_keys_seeded({"bsk": np.zeros(1, U), "ksk": np.zeros(1, U), "pack_key_body": np.zeros(1, U)})
    for gone in ("eval_mask_key", "ksk_body"):
        with pytest.raises(ValueError, match=gone):
            eval_keys_seeded({k: v for k, v in d.items() if k != gone})
    want = seeded_eval_key_sizes(TOY_MB, d)
    assert set(want) == {"bsk_body", "ksk_body", "gadget_bsk1_body", "pack_key_body", "bridge_key_body"}
    assert all(want[k] == d[k].size for k in want)
    for name in want:                                               # a size mismatch names its array
        for bad in (d[name][:-1], np.concatenate([d[name], d[name][:1]])):
            with pytest.raises(ValueError, match="^" + name + ":"):
                seeded_eval_key_sizes(TOY_MB, dict(d, **{name: bad}))
    with pytest.raises(ValueError, match="^bsk_body:"):             # TOY_MB's bodies against TOY
        seeded_eval_key_sizes(TOY, d)
    with pytest.raises(ValueError, match="gadget_bsk1_body"):       # a gadget the parameters have
        seeded_eval_key_sizes(TOY_MB, {k: v for k, v in d.items() if k != "gadget_bsk1_body"})
    for mk in ("eval_mask_key", "pack_mask_key", "bridge_mask_key"):
        with pytest.raises(ValueError, match="^" + mk + ":"):
            seeded_eval_key_sizes(TOY_MB, dict(d, **{mk: d[mk][:7]}))
    with pytest.raises(ValueError, match="pack_key_body without"):
        seeded_eval_key_sizes(TOY_MB, {k: v for k, v in d.items() if k != "pack_mask_key"})
    with pytest.raises(ValueError, match="^pack_key_body:"):        # a gadget the library rejects: 0 words
        seeded_eval_key_sizes(TOY_MB, dict(d, pack_gadget=np.array([8, 3])))
    assert "bridge_key_body" not in seeded_eval_key_sizes(TOY, seeded_dict(TOY, bridge=None))


def test_servers_accept_a_seeded_packing_key():
    """The "no packing key" check of the three servers takes pack_key_body too
    (checked before any device work: a dict without either is refused here)."""
    from fheicp.private import PrivateServer
    from fheicp.query import QueryServer
    from fheicp.stored import CorpusServer
    d = seeded_dict(TOY, pack=None, bridge=None)
    for cls, args in ((QueryServer, (d, None, 8)), (PrivateServer, (d, None, 8)), (CorpusServer, (d, None, 8, None))):
        with pytest.raises(ValueError, match="no packing key"):
            cls(*args)
    srv = CorpusServer.__new__(CorpusServer)
    with pytest.raises(ValueError, match="no packing key"):
        srv.rekey(d)


def test_save_and_load_carry_a_seeded_dict(tmp_path):
    from fheicp.engine import eval_keys_seeded, seeded_eval_key_sizes
    from fheicp.query import load_eval_keys, save_eval_keys
    rng = np.random.default_rng(3)
    d = seeded_dict(TOY_MB)
    for k in d:
        if k.endswith("_body"):
            d[k] = rng.integers(0, 2 ** 64, d[k].size, dtype=U)
    d.update(key_id=np.array(["0123456789abcdef"]), pack_bit_levels=np.array([2], np.int64),
             bridge_from=np.array(["fedcba9876543210"]))
    path = tmp_path / "keys.npz"
    save_eval_keys(str(path), d)
    back = load_eval_keys(str(path))
    assert set(back) == set(d)
    for k in d:
        assert back[k].dtype == np.asarray(d[k]).dtype, k
        np.testing.assert_array_equal(back[k], d[k])
    assert eval_keys_seeded(back) and seeded_eval_key_sizes(TOY_MB, back)
    assert back["eval_mask_key"].dtype == np.uint32
    # a third of the full form's bytes and less: the file is about the bodies
    L = _lib.lib()
    P = _lib.params_struct(TOY_MB.as_dict())
    full = 8 * (L.fhe_bsk_words(C.byref(P)) + L.fhe_ksk_words(C.byref(P)) + L.fhe_fast_bsk_words(C.byref(P), 1) +
                L.fhe_pack_key_words(C.byref(P), 4, 3) + L.fhe_bridge_key_words(C.byref(P), 7, 7))
    assert path.stat().st_size < full / 3 + 8192


# ------------------------------------------------------- host-only contexts --
def test_seeded_key_entry_points_on_host_context():
    """Argument errors first (FHE_E_ARG with "seeded": null keys and buffers, a
    bad gadget, an old key word other than 0 or 1, a missing gadget body), then
    the missing device."""
    L = _lib.lib()
    prm = DEFAULTS                                  # two fast gadgets: gadget bodies 1 and 2 are required
    Pm = _lib.params_struct(prm.as_dict())
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(Pm), -1, C.byref(h)) == 0
    buf = (C.c_uint64 * (prm.k * prm.N))()          # zeros: also a valid old big key
    key = (C.c_uint32 * 8)(*range(8))
    out_key = (C.c_uint32 * 8)()
    gad = (C.c_void_p * 5)(C.addressof(buf), C.addressof(buf), None, None, None)
    gad1 = (C.c_void_p * 5)(C.addressof(buf), None, None, None, None)

    def is_seeded_arg(rc, why):
        assert rc == -1, why
        assert b"seeded" in L.fhe_last_error(h), (why, L.fhe_last_error(h))

    def is_host_only(rc, why):
        assert rc == -2, (why, L.fhe_last_error(h))
        assert b"host-only" in L.fhe_last_error(h), why

    is_host_only(L.fhe_keygen_seeded(h, key, key, None), "keygen")
    is_seeded_arg(L.fhe_keygen_seeded(h, None, key, None), "keygen mask")
    is_seeded_arg(L.fhe_keygen_seeded(h, key, None, None), "keygen noise")
    assert L.fhe_keygen_seeded(None, key, key, None) == -1

    is_host_only(L.fhe_keygen_pack_key_seeded(h, 4, 3, key, key, None), "pack keygen")
    is_seeded_arg(L.fhe_keygen_pack_key_seeded(h, 4, 3, None, key, None), "pack keygen mask")
    is_seeded_arg(L.fhe_keygen_pack_key_seeded(h, 4, 3, key, None, None), "pack keygen noise")
    is_host_only(L.fhe_keygen_bridge_key_seeded(h, buf, 4, 3, key, key, None), "bridge keygen")
    is_seeded_arg(L.fhe_keygen_bridge_key_seeded(h, None, 4, 3, key, key, None), "bridge keygen old key")
    is_seeded_arg(L.fhe_keygen_bridge_key_seeded(h, buf, 4, 3, None, key, None), "bridge keygen mask")
    is_seeded_arg(L.fhe_keygen_bridge_key_seeded(h, buf, 4, 3, key, None, None), "bridge keygen noise")
    two = (C.c_uint64 * (prm.k * prm.N))()
    two[5] = 2
    is_seeded_arg(L.fhe_keygen_bridge_key_seeded(h, two, 4, 3, key, key, None), "bridge keygen old key word 2")

    is_host_only(L.fhe_import_pack_key_seeded(h, 4, 3, key, buf), "pack import")
    is_seeded_arg(L.fhe_import_pack_key_seeded(h, 4, 3, None, buf), "pack import mask")
    is_seeded_arg(L.fhe_import_pack_key_seeded(h, 4, 3, key, None), "pack import body")
    is_host_only(L.fhe_import_bridge_key_seeded(h, 4, 3, key, buf), "bridge import")
    is_seeded_arg(L.fhe_import_bridge_key_seeded(h, 4, 3, None, buf), "bridge import mask")
    is_seeded_arg(L.fhe_import_bridge_key_seeded(h, 4, 3, key, None), "bridge import body")
    for b, lv in ((0, 6), (8, 6), (7, 0), (7, 9), (7, 8)):
        is_seeded_arg(L.fhe_keygen_pack_key_seeded(h, b, lv, key, key, None), ("pack keygen", b, lv))
        is_seeded_arg(L.fhe_keygen_bridge_key_seeded(h, buf, b, lv, key, key, None), ("bridge keygen", b, lv))
        is_seeded_arg(L.fhe_import_pack_key_seeded(h, b, lv, key, buf), ("pack import", b, lv))
        is_seeded_arg(L.fhe_import_bridge_key_seeded(h, b, lv, key, buf), ("bridge import", b, lv))

    is_host_only(L.fhe_import_eval_keys_seeded(h, key, buf, buf, gad), "import")
    is_seeded_arg(L.fhe_import_eval_keys_seeded(h, None, buf, buf, gad), "import mask")
    is_seeded_arg(L.fhe_import_eval_keys_seeded(h, key, None, buf, gad), "import bsk body")
    is_seeded_arg(L.fhe_import_eval_keys_seeded(h, key, buf, None, gad), "import ksk body")
    is_seeded_arg(L.fhe_import_eval_keys_seeded(h, key, buf, buf, None), "import no gadget bodies")
    is_seeded_arg(L.fhe_import_eval_keys_seeded(h, key, buf, buf, gad1), "import gadget 2 missing")
    assert b"gadget 2" in L.fhe_last_error(h)

    is_host_only(L.fhe_export_eval_keys_seeded(h, out_key, buf, buf, gad), "export")
    is_seeded_arg(L.fhe_export_eval_keys_seeded(h, None, buf, buf, gad), "export mask")
    is_seeded_arg(L.fhe_export_eval_keys_seeded(h, out_key, None, buf, gad), "export bsk body")
    is_seeded_arg(L.fhe_export_eval_keys_seeded(h, out_key, buf, None, gad), "export ksk body")
    is_seeded_arg(L.fhe_export_eval_keys_seeded(h, out_key, buf, buf, gad1), "export gadget 2 missing")
    is_host_only(L.fhe_export_pack_key_seeded(h, out_key, buf), "pack export")
    is_seeded_arg(L.fhe_export_pack_key_seeded(h, None, buf), "pack export mask")
    is_seeded_arg(L.fhe_export_pack_key_seeded(h, out_key, None), "pack export body")
    is_host_only(L.fhe_export_bridge_key_seeded(h, out_key, buf), "bridge export")
    is_seeded_arg(L.fhe_export_bridge_key_seeded(h, None, buf), "bridge export mask")
    is_seeded_arg(L.fhe_export_bridge_key_seeded(h, out_key, None), "bridge export body")
    for f in (L.fhe_export_pack_key_seeded, L.fhe_export_bridge_key_seeded):
        assert f(None, out_key, buf) == -1
    L.fhe_ctx_destroy(h)
