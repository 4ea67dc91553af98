"""CPU: the both-private search's seeded payloads, the parts
that need no GPU: the two payload formats and what they refuse, the id-range
and mixed-form checks of a batch and of a server's document blocks, the new
entry points on a host-only context, and the numpy restatement of the
expansion (tests/seeded_private_ref.py) against a hand-assembled full form."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import extprod_ref as X
import seeded_private_ref as S

from fheicp import _lib
from fheicp import private as P
from fheicp.params import TOY, params_for_bits

REPO = Path(__file__).resolve().parents[1]
U = np.uint64
N, K, GADGET, D, B = 256, 2, (7, 6), 16, 37
G = -(-B // (N // D))                                     # 3 document GLWEs, the last partly filled
KEY = np.arange(1, 9, dtype=np.uint32) * np.uint32(0x01020304)
NEW_INT = ("fhe_encrypt_packed_seeded_batch", "fhe_encrypt_ggsw_seeded", "fhe_expand_packed_seeded_batch",
           "fhe_expand_ggsws_seeded", "fhe_glwe_docs_pack_seeded", "fhe_glwe_docs_queries_pack_seeded",
           "fhe_search_ggsw_seeded_batch", "fhe_search_ggsws_seeded_batch")


def seeded_query(id0=5, key=KEY, gadget=GADGET, d=D, n=N, k=K, P0=21, fill=3):
    body = np.full((k + 1) * gadget[1] * n, fill, U)
    return P.pack_ggsw_query_seeded(body, id0, key, d, P0, *gadget, n, k)


def seeded_block(id0=9, key=KEY, b=B, d=D, n=N, k=K, P0=21, fill=4):
    body = np.full(-(-b // (n // d)) * n, fill, U)
    return P.pack_doc_block_seeded(body, id0, key, b, d, P0, n, k)


# ------------------------------------------------------------------- formats --
def test_round_trip_and_exact_sizes():
    beta, L = GADGET
    rng = np.random.default_rng(1)
    qbody = rng.integers(0, 2 ** 64, (K + 1) * L * N, dtype=U)
    dbody = rng.integers(0, 2 ** 64, G * N, dtype=U)
    q = P.pack_ggsw_query_seeded(qbody, 2 ** 64 - 2, KEY, D, 21, beta, L, N, K)
    d = P.pack_doc_block_seeded(dbody, 2 ** 64 - 1, KEY.tobytes(), B, D, 21, N, K)
    assert q.dtype == d.dtype == U
    assert q.size == P.HEADER_WORDS + 1 + 4 + (K + 1) * L * N
    assert d.size == P.HEADER_WORDS + 1 + 4 + G * N
    pq, pd = P.unpack_ggsw_query_seeded(q), P.unpack_doc_block_seeded(d)
    assert (pq["D"], pq["P0"], pq["base_log"], pq["level"], pq["N"], pq["k"], pq["id0"]) == \
        (D, 21, beta, L, N, K, 2 ** 64 - 2)
    assert (pd["B"], pd["D"], pd["P0"], pd["N"], pd["k"], pd["id0"]) == (B, D, 21, N, K, 2 ** 64 - 1)
    for pl, body in ((pq, qbody), (pd, dbody)):
        assert pl["seeded"] is True
        np.testing.assert_array_equal(pl["mask_key"], KEY)
        assert pl["mask_key"].dtype == np.uint32
        np.testing.assert_array_equal(pl["body"], body)
    assert P.unpack_any_query(q)["seeded"] and P.unpack_any_docs(d)["seeded"]
    # the full forms still go through the dispatch, unchanged
    fq = P.pack_ggsw_query(np.zeros((K + 1) * L * (K + 1) * N, U), D, 21, beta, L, N, K)
    fd = P.pack_doc_block(np.zeros(G * (K + 1) * N, U), B, D, 21, N, K)
    assert P.unpack_any_query(fq)["seeded"] is False and P.unpack_any_docs(fd)["seeded"] is False
    # the payload bytes at N = 1024, k = 2, D = 16, gadget (7, 6): a third of the full form beside the header
    n = 1024
    sd = P.pack_doc_block_seeded(np.zeros(n, U), 0, KEY, n // D, D, 21, n, K)          # one document GLWE
    fd = P.pack_doc_block(np.zeros((K + 1) * n, U), n // D, D, 21, n, K)
    assert 8 * (sd.size - P.SEEDED_HEADER_WORDS) == 8192 and 8 * (fd.size - P.HEADER_WORDS) == 24576
    sq = P.pack_ggsw_query_seeded(np.zeros((K + 1) * 6 * n, U), 0, KEY, D, 21, 7, 6, n, K)
    fq = P.pack_ggsw_query(np.zeros((K + 1) * 6 * (K + 1) * n, U), D, 21, 7, 6, n, K)
    assert 8 * (sq.size - P.SEEDED_HEADER_WORDS) == 147456 and 8 * (fq.size - P.HEADER_WORDS) == 442368
    P.unpack_doc_block_seeded(sd), P.unpack_ggsw_query_seeded(sq)


def test_formats_refuse_what_is_not_theirs():
    from fheicp.corpus import pack_payload, unpack_payload
    from fheicp.query import pack_query, pack_reply, unpack_query
    beta, L = GADGET
    q, d = seeded_query(), seeded_block()
    fq = P.pack_ggsw_query(np.zeros((K + 1) * L * (K + 1) * N, U), D, 21, beta, L, N, K)
    fd = P.pack_doc_block(np.zeros(G * (K + 1) * N, U), B, D, 21, N, K)
    others = [pack_query(np.zeros(D, U), 3, 21, KEY, K * N), pack_payload(np.zeros(D + 1, U), 3, 21, KEY, K * N),
              pack_reply(np.zeros((K + 1) * N, U), np.zeros((K + 1) * N, U), 4, 21, 0)]
    for unpack, good, full in ((P.unpack_ggsw_query_seeded, q, fq), (P.unpack_doc_block_seeded, d, fd)):
        unpack(good)
        for bad in (good[:-1], good[:P.SEEDED_HEADER_WORDS - 1], np.concatenate([good, good[-1:]]),    # sizes
                    good.astype(np.int64), good.astype(np.float64), good.reshape(1, -1),              # dtype, shape
                    full, q if good is d else d, *others):                                            # other magics
            with pytest.raises(ValueError):
                unpack(bad)
        wrong = good.copy()
        wrong[0] ^= U(1)
        with pytest.raises(ValueError, match="not an fheicp seeded"):
            unpack(wrong)
        v2 = good.copy()
        v2[1] = 2
        with pytest.raises(ValueError, match="version 2"):
            unpack(v2)
    # D = 257 does not fit one GLWE of N = 256, in either format
    with pytest.raises(ValueError, match="D = 257"):
        P.unpack_ggsw_query_seeded(seeded_query(d=257))
    big = P.pack_doc_block_seeded(np.zeros(N, U), 0, KEY, 1, 257, 21, N, K)
    with pytest.raises(ValueError, match="D = 257"):
        P.unpack_doc_block_seeded(big)
    # and nothing else parses a seeded payload
    for unpack in (P.unpack_ggsw_query, P.unpack_doc_block, unpack_query, unpack_payload):
        for s in (q, d):
            with pytest.raises(ValueError):
                unpack(s)
    with pytest.raises(ValueError, match="32 bytes"):
        P.pack_doc_block_seeded(np.zeros(N, U), 0, KEY[:7], 1, D, 21, N, K)


# ------------------------------------------------------------ overlap checks --
def test_id_ranges_overlap_modulo_2_64():
    f = P.id_ranges_overlap
    assert f(10, 5, 14, 1) and f(14, 1, 10, 5) and not f(10, 5, 15, 1) and not f(15, 1, 10, 5)
    assert f(2 ** 64 - 2, 4, 1, 3) and f(1, 3, 2 ** 64 - 2, 4)          # [2^64 - 2, 2) wraps onto 1
    assert not f(2 ** 64 - 2, 4, 2, 3) and f(2 ** 64 - 1, 1, 2 ** 64 - 1, 1)
    assert not f(0, 0, 0, 5)
    span = P.ggsw_id_span(K, GADGET[1])
    ids = P.ggsw_query_ids(2 ** 64 - span - 1, 3, K, GADGET[1])        # the client's own ranges never meet
    assert not any(f(a, span, b, span) for i, a in enumerate(ids) for b in ids[:i])


def test_check_query_batch_names_the_query():
    span = P.ggsw_id_span(K, GADGET[1])
    un = P.unpack_any_query
    ok = [un(seeded_query(id0=i)) for i in P.ggsw_query_ids(2 ** 64 - span - 3, 3, K, GADGET[1])]
    assert P.check_query_batch(ok) is True
    beta, L = GADGET
    full = un(P.pack_ggsw_query(np.zeros((K + 1) * L * (K + 1) * N, U), D, 21, beta, L, N, K))
    assert P.check_query_batch([full, full]) is False
    with pytest.raises(ValueError, match="query 2: a full-form payload"):
        P.check_query_batch([ok[0], ok[1], full])
    with pytest.raises(ValueError, match="query 1: a seeded payload"):
        P.check_query_batch([full, ok[0]])
    other = un(seeded_query(id0=10 ** 6, key=KEY[::-1].copy()))
    with pytest.raises(ValueError, match="query 2: mask key"):
        P.check_query_batch([ok[0], ok[1], other])
    with pytest.raises(ValueError, match="query 1: stream ids"):
        P.check_query_batch([un(seeded_query(id0=100)), un(seeded_query(id0=100 + span - 1))])
    P.check_query_batch([un(seeded_query(id0=100)), un(seeded_query(id0=100 + span))])
    # a range that wraps past 2^64 meets one that starts at 0
    with pytest.raises(ValueError, match="query 2: stream ids"):
        P.check_query_batch([un(seeded_query(id0=2 ** 64 - 2)), un(seeded_query(id0=5000)), un(seeded_query(id0=1))])
    with pytest.raises(ValueError, match="query 1: gadget level"):
        P.check_query_batch([ok[0], un(seeded_query(id0=7777, gadget=(7, 5)))])
    with pytest.raises(ValueError, match="empty"):
        P.check_query_batch([])


def test_server_tracks_document_ids_per_mask_key():
    """PrivateServer's record of the seeded blocks it packed: ids must not
    repeat under one mask key; the same block again (the other operand) passes."""
    srv = P.PrivateServer.__new__(P.PrivateServer)         # the bookkeeping alone: no engine, no keys
    srv._seeded_docs = {}
    note = lambda **kw: srv._note_seeded_docs(P.unpack_doc_block_seeded(seeded_block(**kw)))
    note(id0=2 ** 64 - 2)                                  # 3 GLWEs: ids 2^64 - 2, 2^64 - 1, 0
    note(id0=2 ** 64 - 2)                                  # the same block, packed for the other operand
    note(id0=1)                                            # 1, 2, 3
    note(id0=0, key=KEY[::-1].copy())                      # another mask key: its own id space
    for bad in (0, 3, 2 ** 64 - 4):
        with pytest.raises(ValueError, match="document block: stream ids"):
            note(id0=bad)
    with pytest.raises(ValueError, match="document block: stream ids"):
        note(id0=2 ** 64 - 2, fill=5)                      # the same ids under other contents
    note(id0=4)


# ------------------------------------------------------- host-only contexts --
def test_new_exports_present_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fhe_icp.h").read_text(), flags=re.S)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    integ = (REPO / "integration" / "fhe_gpu.py").read_text()
    guide = (REPO / "INTEGRATION.md").read_text()
    L = _lib.lib()
    for name in NEW_INT + ("fhe_ggsw_body_words",):
        ret = "int" if name in NEW_INT else "size_t"
        m = re.search(r"^" + ret + " " + name + r"\((.*?)\);", hdr, flags=re.S | re.M)
        assert m, name
        assert len(bound[name]) == m.group(1).count(",") + 1, name    # one ctypes argument per C parameter
        assert hasattr(L, name)
        assert f'"{name}"' in integ and name in guide
    assert hdr.index("fhe_search_ggsws_group_batch") < min(hdr.index(n) for n in NEW_INT)     # appended
    from fheicp.engine import Engine
    for meth in ("encrypt_docs_glwe_seeded", "encrypt_ggsw_seeded", "expand_docs_glwe_seeded", "expand_ggsws_seeded",
                 "pack_docs_glwe_seeded", "search_ggsw_seeded", "search_ggsws_seeded", "ggsw_body_words"):
        assert callable(getattr(Engine, meth))


def test_ggsw_body_words():
    L = _lib.lib()
    for prm in (TOY, params_for_bits(21)):
        Pm = _lib.params_struct(prm.as_dict())
        for beta in range(0, 9):
            for lv in range(0, 10):
                full = L.fhe_ggsw_words(C.byref(Pm), beta, lv)
                body = L.fhe_ggsw_body_words(C.byref(Pm), beta, lv)
                if full == 0:                              # a rejected gadget
                    assert body == 0, (beta, lv)
                else:
                    assert body * (prm.k + 1) == full and body == (prm.k + 1) * lv * prm.N, (beta, lv)
    assert L.fhe_ggsw_words(C.byref(Pm), 7, 6) > 0 and L.fhe_ggsw_body_words(C.byref(Pm), 7, 8) == 0
    assert L.fhe_ggsw_body_words(None, 7, 6) == 0
    assert params_for_bits(21).N == 1024
    p21 = _lib.params_struct(params_for_bits(21).as_dict())
    assert L.fhe_ggsw_body_words(C.byref(p21), 7, 6) * 8 == 147456       # against 442,368 bytes in full form


def test_seeded_entry_points_on_host_context():
    """Argument errors first (FHE_E_ARG with "seeded", null keys among them: a
    host-only context reports them too), then the missing device."""
    L = _lib.lib()
    prm = params_for_bits(21)
    Pm = _lib.params_struct(prm.as_dict())
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(Pm), -1, C.byref(h)) == 0
    buf = (C.c_uint64 * 64)()      # stands for every device buffer: nothing reads it on a host-only context
    hv = (C.c_int64 * 4)()
    key = (C.c_uint32 * 8)(*range(8))

    calls = {
        "fhe_encrypt_packed_seeded_batch":
            lambda mk=key, nk=key, Bn=4, Dn=16, a=buf, o=buf, **_: L.fhe_encrypt_packed_seeded_batch(
                h, a, Bn, Dn, mk, nk, 0, o, None),
        "fhe_encrypt_ggsw_seeded":
            lambda mk=key, nk=key, Dn=16, b=7, lv=6, a=buf, o=buf, **_: L.fhe_encrypt_ggsw_seeded(
                h, a, Dn, b, lv, mk, nk, 0, o, None),
        "fhe_expand_packed_seeded_batch":
            lambda mk=key, Bn=4, Dn=16, a=buf, o=buf, **_: L.fhe_expand_packed_seeded_batch(
                h, a, 0, Bn, Dn, mk, o, None),
        "fhe_expand_ggsws_seeded":
            lambda mk=key, Q=2, b=7, lv=6, a=buf, o=buf, **_: L.fhe_expand_ggsws_seeded(h, a, buf, Q, b, lv, mk, o, None),
        "fhe_glwe_docs_pack_seeded":
            lambda mk=key, Bn=4, Dn=16, b=7, lv=6, a=buf, o=buf, **_: L.fhe_glwe_docs_pack_seeded(
                h, a, 0, Bn, Dn, b, lv, mk, o, None),
        "fhe_glwe_docs_queries_pack_seeded":
            lambda mk=key, Bn=4, Dn=16, b=7, lv=6, a=buf, o=buf, **_: L.fhe_glwe_docs_queries_pack_seeded(
                h, a, 0, Bn, Dn, b, lv, mk, o, None),
        "fhe_search_ggsw_seeded_batch":
            lambda mk=key, Bn=4, Dn=16, b=7, lv=6, a=buf, o=buf, **_: L.fhe_search_ggsw_seeded_batch(
                h, a, 0, b, lv, mk, buf, Bn, Dn, 0, 0, 0, o, buf, None),
        "fhe_search_ggsws_seeded_batch":
            lambda mk=key, Q=2, Bn=4, Dn=16, b=7, lv=6, a=buf, o=buf, **_: L.fhe_search_ggsws_seeded_batch(
                h, a, buf, b, lv, mk, buf, Q, Bn, Dn, 0, hv, 0, o, buf, None),
    }
    assert set(calls) == set(NEW_INT)

    def is_seeded_arg(rc, why):
        assert rc == -1, why
        assert b"seeded" in L.fhe_last_error(h), (why, L.fhe_last_error(h))

    for name, f in calls.items():
        assert f() == -2, name                                          # FHE_E_DEVICE
        assert b"host-only" in L.fhe_last_error(h), name
        is_seeded_arg(f(mk=None), (name, "null mask key"))
        if "encrypt" in name:
            is_seeded_arg(f(nk=None), (name, "null noise key"))
        is_seeded_arg(f(a=None), (name, "null input"))
        is_seeded_arg(f(o=None), (name, "null output"))
        if name != "fhe_expand_ggsws_seeded":
            is_seeded_arg(f(Dn=0), (name, "D = 0"))
        if "packed" not in name:                                        # the entries that take a gadget
            for b, lv in ((0, 6), (8, 6), (7, 0), (7, 9), (7, 8)):
                is_seeded_arg(f(b=b, lv=lv), (name, b, lv))
        if "packed" not in name and name != "fhe_expand_ggsws_seeded":
            is_seeded_arg(f(Dn=prm.N + 1), (name, "D > N"))
        if name not in ("fhe_encrypt_ggsw_seeded", "fhe_expand_ggsws_seeded", "fhe_search_ggsws_seeded_batch"):
            is_seeded_arg(f(Bn=-1), (name, "B < 0"))
    for Q in (0, -1, 65536):
        is_seeded_arg(calls["fhe_expand_ggsws_seeded"](Q=Q), ("expand", Q))
        is_seeded_arg(calls["fhe_search_ggsws_seeded_batch"](Q=Q), ("search", Q))
    for Bn in (0, -3, 2 ** 31):
        is_seeded_arg(calls["fhe_search_ggsws_seeded_batch"](Bn=Bn), ("search", Bn))
        is_seeded_arg(calls["fhe_glwe_docs_queries_pack_seeded"](Bn=Bn), ("pack", Bn))
    assert L.fhe_search_ggsws_seeded_batch(None, buf, buf, 7, 6, key, buf, 2, 4, 16, 0, hv, 0, buf, buf, None) == -1
    nm = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"expand_ggsw_seeded", nm, 64) == 0 and nm.value == b""
    L.fhe_ctx_destroy(h)


# --------------------------------------------------------------- restatement --
@pytest.mark.parametrize("gadget", [(4, 3), (7, 7)])
def test_restatement_expansion_feeds_the_external_product(oracle_lib, gadget):
    """For body arrays and a mask key, the restatement's expansion equals a
    full form assembled by hand (every mask word fetched on its own through the
    oracle's block function, placed by the addressing rule of §8.15), and so
    does its product under tests/extprod_ref.py. N = 64, the scheme's k, ids
    that wrap."""
    beta, L = gadget
    n, k, Gn = 64, TOY.k, 2
    rng = np.random.default_rng(17 * beta + L)
    key = oracle_lib.key_from_seed(1234 + beta)
    qbody = rng.integers(0, 2 ** 64, ((k + 1) * L, n), dtype=U)
    dbody = rng.integers(0, 2 ** 64, (Gn, n), dtype=U)
    qid, did = 2 ** 64 - 5, 2 ** 64 - 1                   # both ranges cross the wrap

    def word(tag, ident, w):
        ident %= 2 ** 64
        o = oracle_lib.chacha20_block(key, w >> 3, np.array([tag, ident & 0xFFFFFFFF, ident >> 32], np.uint32))
        return int(o[2 * (w & 7)]) | (int(o[2 * (w & 7) + 1]) << 32)

    ggsw = np.zeros((k + 1, L, k + 1, n), U)
    for c in range(k + 1):
        for l in range(L):
            r = c * L + l
            for cp in range(k):
                ggsw[c, l, cp] = [word(S.TAG_GGSW_MASK, qid + r * k + cp, t) for t in range(n)]
            ggsw[c, l, k] = qbody[r]
    glwe = np.zeros((Gn, k + 1, n), U)
    for g in range(Gn):
        for i in range(k):
            glwe[g, i] = [word(S.TAG_ENC_MASK, did + g, i * n + t) for t in range(n)]
        glwe[g, k] = dbody[g]
    eg, ed = S.expand_ggsw(qbody, key, qid, n, k, L), S.expand_glwe(dbody, key, did, n, k)
    np.testing.assert_array_equal(eg, ggsw)
    np.testing.assert_array_equal(ed, glwe)
    np.testing.assert_array_equal(X.external_product(ed, eg, beta), X.external_product(glwe, ggsw, beta))
    # the masks are uniform words: on every level their digits take both signs
    neg, pos = S.digit_signs(ed[:, :k], beta, L)
    assert neg.all() and pos.all()
