"""CPU: the both-private search for several GGSW queries —
the transposed product restated in numpy against tests/extprod_ref.py, the new
entry points' exports and validation on a host-only context, the workspace
bound (nothing proportional to ((k+1)N)^2), the batch check and the stream-id
ranges of a batch of queries."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import extprod_ref as X
from pack_ref import decompose_ks_np

from fheicp import _lib
from fheicp.params import TOY, params_for_bits

REPO = Path(__file__).resolve().parents[1]
U = np.uint64
GADGETS = [(4, 3), (7, 7)]
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0, 1 << 63)   # tests/test_gpu_extprod.py's
NEW_INT = ("fhe_glwe_docs_queries_pack", "fhe_linear_ggsws_batch", "fhe_compare_ggsws_batch",
           "fhe_search_ggsws_batch")
NEW_SIZE = ("fhe_glwe_docs_queries_bytes", "fhe_ggsws_ws_bytes")


def byte_planes(x) -> np.ndarray:
    """The balanced byte split of k_extprod_planes: s_p = (int8)(x & 0xff),
    x = (x - s_p) >> 8; int64 [8, ...]."""
    x = np.asarray(x, dtype=U).copy()
    out = []
    with np.errstate(over="ignore"):
        for _ in range(8):
            s = (x & U(0xFF)).astype(np.uint8).view(np.int8).astype(np.int64)
            x = (x - s.astype(U)) >> U(8)
            out.append(s)
    assert x.max() <= 1                                 # what is left is the carry out of bit 63: 0 mod 2^64
    return np.stack(out)


def transposed_product(glwe, ggsws, beta: int) -> np.ndarray:
    """out[q][g][c'][t] = sum_p 2^(8p) sum_{c,l,s} plane_p(Row_q(c,l)[c'][s]) E_{g,c,l}[t - s],
    E[m] = d[m] for m >= 0, -d[m + N] for m < 0, from i8 operands and wide
    integer sums: [Q, G, k+1, N]."""
    ggsws = np.asarray(ggsws, dtype=U)
    Qn, k1, L, _, N = ggsws.shape
    glwe = np.asarray(glwe, dtype=U).reshape(-1, k1, N)
    G = len(glwe)
    d = decompose_ks_np(glwe.reshape(G, k1 * N), beta, L).reshape(G, k1, N, L)
    assert np.abs(d).max() <= 64                        # negating an int8 digit is exact
    d = np.moveaxis(d, 3, 2)                            # [G, c, l, N]
    E = np.concatenate([-d, d], axis=-1)                # E[m] at index m + N, m in [-N, N)
    t, s = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    Et = E[..., t - s + N]                              # [G, c, l, t, s]
    planes = byte_planes(ggsws)                         # [8, Q, c, l, c', s]
    assert planes.min() >= -128 and planes.max() <= 127
    acc = np.einsum("pqclas,gclts->pqgat", planes, Et)  # exact: |sum| < 2^31
    assert np.abs(acc).max() < 2 ** 31
    out = np.zeros(acc.shape[1:], U)
    with np.errstate(over="ignore"):
        for p in range(8):
            out += acc[p].astype(U) << U(8 * p)
    return out


@pytest.mark.parametrize("gadget", GADGETS)
def test_transposed_product_equals_external_product(gadget):
    """The identity the batched GEMM computes, at the scheme's k with N = 64,
    Q = 3, G = 2, edge words in rows and documents and tie inputs with both
    coins on every level."""
    beta, L = gadget
    k1, N, Qn, G = TOY.k + 1, 64, 3, 2
    rng = np.random.default_rng(1000 * beta + L)
    ggsws = rng.integers(0, 2 ** 64, (Qn, k1, L, k1, N), dtype=U)
    glwe = rng.integers(0, 2 ** 64, (G, k1, N), dtype=U)
    for i, w in enumerate(EDGE_WORDS):
        ggsws[i % Qn, i % k1, i % L, (i + 1) % k1, 3 * i:3 * i + 2] = U(w)
        glwe[i % G, i % k1, 5 * i:5 * i + 3] = U(w)
    prec = beta * L
    ties = [((1 << (beta - 1)) << (64 - beta * l)) | (c << (62 - prec - (L - l))) for l in range(1, L + 1)
            for c in (0, 1)]
    glwe[1, k1 - 1, 30:30 + len(ties)] = np.array(ties, U)
    got = transposed_product(glwe, ggsws, beta)
    for q in range(Qn):
        np.testing.assert_array_equal(got[q], X.external_product(glwe, ggsws[q], beta))


def test_new_exports_present_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fhe_icp.h").read_text(), flags=re.S)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    integ = (REPO / "integration" / "fhe_gpu.py").read_text()
    guide = (REPO / "INTEGRATION.md").read_text()
    L = _lib.lib()
    for name in NEW_INT + NEW_SIZE:
        ret = "int" if name in NEW_INT else "size_t"
        m = re.search(r"^" + ret + " " + name + r"\((.*?)\);", hdr, flags=re.S | re.M)
        assert m, name
        assert name in bound, name
        assert len(bound[name]) == m.group(1).count(",") + 1, name    # one ctypes argument per C parameter
        assert hasattr(L, name)
        assert f'"{name}"' in integ and name in guide
    # appended after the §8.9 block
    assert hdr.index("fhe_search_seeded_queries_batch") < min(hdr.index(n) for n in NEW_INT + NEW_SIZE)
    from fheicp.engine import Engine
    for meth in ("pack_docs_glwe_queries", "linear_ggsws", "compare_ggsws", "search_ggsws"):
        assert callable(getattr(Engine, meth))
    from fheicp.private import PrivateClient, PrivateServer, check_ggsw_batch
    assert callable(PrivateClient.encrypt_queries) and PrivateClient.encrypt_queries.__qualname__.startswith("Private")
    assert callable(PrivateServer.pack_docs_many) and callable(PrivateServer.search_many)
    assert callable(check_ggsw_batch)


def test_ggsw_queries_entry_points_on_host_context():
    """Argument errors first (FHE_E_ARG with "ggsw queries", a host-only
    context reports them too), null pointers included; then the missing
    device."""
    L = _lib.lib()
    prm = params_for_bits(21)
    P = _lib.params_struct(prm.as_dict())
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(P), -1, C.byref(h)) == 0
    buf = (C.c_uint64 * 64)()      # stands for every device buffer: nothing reads it on a host-only context
    hv = (C.c_int64 * 4)()

    def lin(Q, B, D, b=7, lv=6, g=buf, d=buf, hc=hv, out=buf):
        return L.fhe_linear_ggsws_batch(h, g, b, lv, d, Q, B, D, hc, out, None)

    def cmp_(Q, B, D, b=7, lv=6, g=buf, d=buf, hT=hv, out=buf):
        return L.fhe_compare_ggsws_batch(h, g, b, lv, d, Q, B, D, 0, hT, out, buf, None)

    def sea(Q, B, D, b=7, lv=6, g=buf, d=buf, hT=hv, out=buf, lb=0):
        return L.fhe_search_ggsws_batch(h, g, b, lv, d, Q, B, D, 0, hT, lb, out, buf, None)

    for f in (lin, cmp_, sea):
        for Qn, B, D in ((0, 4, 16), (-1, 4, 16), (2, 0, 16), (2, -3, 16), (2, 4, 0), (2, 4, -1), (2, 4, prm.N + 1),
                         (65536, 4, 16), (65535, 2 ** 16, 1), (2, 2 ** 31, 16)):
            assert f(Qn, B, D) == -1, (Qn, B, D)
            assert b"ggsw queries" in L.fhe_last_error(h), L.fhe_last_error(h)
        for b, lv in ((0, 6), (8, 6), (7, 0), (7, 9), (7, 8)):          # (7, 8): level (base_log + 1) > 62
            assert f(2, 4, 16, b, lv) == -1, (b, lv)
            assert b"ggsw queries" in L.fhe_last_error(h)
        for nulls in ({"g": None}, {"d": None}, {"out": None}, {"hc" if f is lin else "hT": None}):
            assert f(2, 4, 16, **nulls) == -1, nulls
            assert b"ggsw queries" in L.fhe_last_error(h)
        assert f(2, 4, 16) == -2
        assert b"host-only" in L.fhe_last_error(h)
    assert sea(2, 4, 16, lb=9) == -1 and sea(2, 4, 16, lb=-1) == -1
    assert b"ggsw queries" in L.fhe_last_error(h)
    assert L.fhe_linear_ggsws_batch(None, buf, 7, 6, buf, 2, 4, 16, hv, buf, None) == -1
    # the document packer: the same argument rules
    for B, D, b, lv in ((0, 16, 7, 6), (4, 0, 7, 6), (4, prm.N + 1, 7, 6), (4, 16, 8, 6), (4, 16, 7, 9)):
        assert L.fhe_glwe_docs_queries_pack(h, buf, B, D, b, lv, buf, None) == -1
        assert b"ggsw queries" in L.fhe_last_error(h)
    assert L.fhe_glwe_docs_queries_pack(h, None, 4, 16, 7, 6, buf, None) == -1
    assert L.fhe_glwe_docs_queries_pack(h, buf, 4, 16, 7, 6, None, None) == -1
    assert L.fhe_glwe_docs_queries_pack(h, buf, 4, 16, 7, 6, buf, None) == -2
    nm = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"linear_ggsws", nm, 64) == 0 and nm.value == b""
    L.fhe_ctx_destroy(h)


def test_workspace_has_no_toeplitz_operand():
    """At the real parameters, gadget (7, 6), Q = 8, B = 1024, D = 16: the
    batched call's workspace is below 8 (2 * 8 * ggsw_words + 2 G (k+1)N 8)
    bytes, a few MB where Q Toeplitz operands would be 8 * 8 ((k+1)N)^2 L."""
    L = _lib.lib()
    prm = params_for_bits(21)
    P = _lib.params_struct(prm.as_dict())
    Qn, B, D, lv = 8, 1024, 16, 6
    G = -(-B // (prm.N // D))
    n1 = (prm.k + 1) * prm.N
    words = L.fhe_ggsw_words(C.byref(P), 7, lv)
    assert words == (prm.k + 1) * lv * n1
    ws = L.fhe_ggsws_ws_bytes(C.byref(P), Qn, B, D, lv)
    assert 0 < ws < 8 * (2 * 8 * words + 2 * G * n1 * 8)
    assert ws < (8 * n1 * n1 * lv) // 16                               # not one query's Toeplitz planes, by far
    # the document operand: 2N + 16 bytes per (GLWE, component, level)
    assert L.fhe_glwe_docs_queries_bytes(C.byref(P), B, D, lv) == G * (prm.k + 1) * lv * (2 * prm.N + 16)
    for bad in ((0, B, D, lv), (Qn, 0, D, lv), (Qn, B, 0, lv), (Qn, B, prm.N + 1, lv), (Qn, B, D, 0), (Qn, B, D, 9)):
        assert L.fhe_ggsws_ws_bytes(C.byref(P), *bad) == 0


def _payload(**over):
    pl = {"D": 16, "P0": 21, "base_log": 7, "level": 6, "N": 2048, "k": 2, "ggsw": np.zeros(4, U)}
    pl.update(over)
    return pl


def test_check_ggsw_batch_names_the_query():
    from fheicp.private import check_ggsw_batch
    check_ggsw_batch([_payload(), _payload(), _payload()])
    check_ggsw_batch([_payload()])
    for field, val in (("D", 8), ("P0", 20), ("base_log", 6), ("level", 7), ("N", 1024), ("k", 1)):
        with pytest.raises(ValueError, match="query 2"):
            check_ggsw_batch([_payload(), _payload(), _payload(**{field: val}), _payload()])
    with pytest.raises(ValueError, match="empty"):
        check_ggsw_batch([])


def test_encrypt_queries_id_ranges_do_not_overlap():
    """Query q's GGSW consumes mask ids id0_q + [0, (k+1) L k) and noise ids
    id0_q + [0, (k+1) L) (k_encrypt_ggsw); the batch's ranges are disjoint
    modulo 2^64, also across the wrap."""
    from fheicp.private import ggsw_id_span, ggsw_query_ids
    for k, lv in ((2, 6), (1, 8), (3, 1)):
        span = ggsw_id_span(k, lv)
        assert span == (k + 1) * lv * k >= (k + 1) * lv
        for id0 in (0, 12345, 2 ** 64 - 3 * span - 1, 2 ** 64 - 1):
            ids = ggsw_query_ids(id0, 8, k, lv)
            assert ids[0] == id0 and len(ids) == 8
            mask = [(i + j) % 2 ** 64 for i in ids for j in range(span)]
            noise = [(i + j) % 2 ** 64 for i in ids for j in range((k + 1) * lv)]
            assert len(set(mask)) == len(mask) and len(set(noise)) == len(noise)
            assert all(0 <= i < 2 ** 64 for i in ids)
