"""CPU: stored-ciphertext search for several queries and two parties
(fheicp.corpus plan_many, fheicp.stored) — the new entry
points' exports and validation on a host-only context, the batch's width
rule, version-2 replies at a width below P0, the reply-width check and the
l1 bound behind CorpusClient's default in_var."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.params import params_for_bits
from fheicp.query import pack_replies, unpack_replies

REPO = Path(__file__).resolve().parents[1]
NEW = ("fhe_linear_seeded_queries_batch", "fhe_compare_seeded_queries_batch", "fhe_search_seeded_queries_batch")
WIDTHS = [20, 19, 19, 19, 19, 21, 15, 4]


def test_new_exports_present_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fhe_icp.h").read_text(), flags=re.S)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    integ = (REPO / "integration" / "fhe_gpu.py").read_text()
    guide = (REPO / "INTEGRATION.md").read_text()
    L = _lib.lib()
    for name in NEW:
        m = re.search(r"^int " + name + r"\((.*?)\);", hdr, flags=re.S | re.M)
        assert m, name
        assert name in bound, name
        assert len(bound[name]) == m.group(1).count(",") + 1, name    # one ctypes argument per C parameter
        assert hasattr(L, name)
        assert f'"{name}"' in integ and name in guide
    # appended after the §8.8 block
    assert hdr.index("fhe_search_queries_batch") < min(hdr.index(n) for n in NEW)
    from fheicp.engine import Engine
    for meth in ("linear_seeded_queries", "compare_seeded_queries", "search_seeded_queries"):
        assert callable(getattr(Engine, meth))
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusServer
    assert callable(EncryptedCorpus.plan_many) and callable(EncryptedCorpus.compare_many)
    assert callable(CorpusClient.decrypt_replies) and callable(CorpusServer.search_many)


def test_seeded_queries_entry_points_on_host_context():
    """Argument errors first (FHE_E_ARG with "seeded queries", a host-only
    context reports them too), null pointers included; then the missing
    device."""
    L = _lib.lib()
    P = _lib.params_struct(params_for_bits(16).as_dict())
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(P), -1, C.byref(h)) == 0
    key = (C.c_uint32 * 8)()
    buf = (C.c_uint64 * 64)()      # stands for every device buffer: nothing reads it on a host-only context
    hv = (C.c_int64 * 4)()

    def lin(Q, B, D, W=buf, hc=hv):
        return L.fhe_linear_seeded_queries_batch(h, buf, buf, B, D, key, Q, W, hc, buf, None)

    def cmp_(Q, B, D, W=buf, hT=hv):
        return L.fhe_compare_seeded_queries_batch(h, buf, buf, B, D, key, Q, W, 0, hT, buf, buf, None)

    def sea(Q, B, D, W=buf, hT=hv, lb=0):
        return L.fhe_search_seeded_queries_batch(h, buf, buf, B, D, key, Q, W, 0, hT, lb, buf, buf, None)

    for f in (lin, cmp_, sea):
        for Qn, B, D in ((0, 4, 16), (-1, 4, 16), (2, 0, 16), (2, -3, 16), (2, 4, 0), (65536, 4, 16),
                         (2, 2 ** 27, 32), (65535, 2 ** 16, 1)):
            assert f(Qn, B, D) == -1, (Qn, B, D)
            assert b"seeded queries" in L.fhe_last_error(h), L.fhe_last_error(h)
        assert f(2, 4, 16, None) == -1                                # null d_W
        assert b"seeded queries" in L.fhe_last_error(h)
        assert f(2, 4, 16, buf, None) == -1                           # null h_cst / h_T
        assert b"seeded queries" in L.fhe_last_error(h)
        assert f(2, 4, 16) == -2
        assert b"host-only" in L.fhe_last_error(h)
    assert sea(2, 4, 16, lb=9) == -1 and sea(2, 4, 16, lb=-1) == -1
    assert L.fhe_linear_seeded_queries_batch(h, None, buf, 4, 16, key, 2, buf, hv, buf, None) == -1
    assert L.fhe_linear_seeded_queries_batch(h, buf, buf, 4, 16, None, 2, buf, hv, buf, None) == -1
    assert L.fhe_linear_seeded_queries_batch(None, buf, buf, 4, 16, key, 2, buf, hv, buf, None) == -1
    nm = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"linear_seeded", nm, 64) == 0 and nm.value == b""
    L.fhe_ctx_destroy(h)


@pytest.fixture(scope="module")
def model16():
    """The 16-dim n_bits = 6 model of tests/test_gpu_corpus.py's corpus16,
    uncompiled (planning needs no device): P0 = 21, q_w = 31 everywhere,
    q_b = 0."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, 6)
    oq = Q.fit_quantized_linear(X, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq)
    assert c.P0 == 21 and cq.q_b == 0 and list(cq.model.q_w) == [31] * 16
    q21, docs = Q.make_corpus(16, 130, seed=21)
    queries = [q21] + [Q.make_corpus(16, 130, seed=s)[0] for s in (31, 32, 33, 34)]
    queries += [np.full(16, -10.0, np.float32), (0.05 * q21).astype(np.float32), np.zeros(16, np.float32)]
    return c, oq, np.stack(queries), docs


def test_plan_many_width_rule(model16):
    c, oq, queries, docs = model16
    P0 = c.P0
    singles = [c.query_plan(q, 0.5) for q in queries]
    assert [p[3] for p in singles] == WIDTHS
    ref = np.stack([Q.corpus_accumulate(oq, c.cq.s_e, 6, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, c.cq.s_e)) * ref.astype(np.float64)
    # the median balance the GPU test relies on: 65 of 130 below for the
    # first seven queries, none for the zero query
    med = [float(np.median(s)) for s in scores]
    assert [int((scores[q] < med[q]).sum()) for q in range(8)] == [65] * 7 + [0]
    keep7 = [q for q in range(8) if q != 5]
    for idx, wantP in ((list(range(8)), 21), (keep7, 20)):
        for ts in (0.5, [med[q] for q in idx], None):
            Wr, cst, Ts, P = c.plan_many(queries[idx], ts)
            assert P == wantP and cst == c.cq.q_b
            assert Wr.dtype == np.int64 and Wr.shape == (len(idx), 16) and len(Ts) == len(idx)
            tl = ts if isinstance(ts, list) else [ts] * len(idx)
            for i, q in enumerate(idx):
                W = c.cq.weights(c.cq.quant(queries[q]))
                np.testing.assert_array_equal(Wr[i], W << (P0 - P))
                _, _, T1, P1 = c.query_plan(queries[q], tl[i])
                assert Ts[i] == T1 and P1 == WIDTHS[q] <= P
                v = ref[q] - Ts[i]
                assert -(2 ** (P - 1)) <= v.min() and v.max() < 2 ** (P - 1)
                assert -(2 ** (P1 - 1)) <= v.min() and v.max() < 2 ** (P1 - 1)
    assert wantP < P0                                                 # the second batch is the rescaled path
    with pytest.raises(ValueError, match="2 thresholds for 8"):
        c.plan_many(queries, [0.1, 0.2])
    with pytest.raises(ValueError, match="empty"):
        c.plan_many(np.zeros((0, 16)), 0.5)


def test_reply_v2_round_trip_below_p0():
    N, N1, P0, P = 1024, 3072, 21, 20
    Qn, B = 7, 130
    G = -(-(Qn * B) // N)
    ga = np.arange(G * N1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    gb = ga[::-1].copy()
    Ts = [-5000, 0, 17, 2 ** 19, -(2 ** 19), 1, -1]
    r = pack_replies(ga, gb, B, P, Ts)
    u = unpack_replies(r, N1, N)
    assert (u["P0"], u["B"], u["Q"], u["T"]) == (P, B, Qn, Ts) and P < P0
    np.testing.assert_array_equal(u["glwe_acc"], ga)
    np.testing.assert_array_equal(u["glwe_bit"], gb)


def test_parse_replies_refuses_widths_outside_4_p0():
    """CorpusClient.decrypt_replies' parsing layer, no device."""
    from fheicp.stored import parse_replies
    N, N1, P0 = 1024, 3072, 21
    g = np.zeros(N1, np.uint64)
    ok = [pack_replies(g, g, 100, P, [3, -3]) for P in (4, 20, P0)]
    got = parse_replies(ok, P0, N1, N)
    assert [r["P0"] for r in got] == [4, 20, P0] and got[0]["T"] == [3, -3]
    assert parse_replies(ok[1], P0, N1, N)[0]["P0"] == 20             # one reply, not in a list
    for bad in (3, P0 + 1):
        with pytest.raises(ValueError, match=f"width {bad}"):
            parse_replies([ok[0], pack_replies(g, g, 100, bad, [3, -3])], P0, N1, N)
    with pytest.raises(ValueError, match="size"):
        parse_replies([pack_replies(g[:-2], g[:-2], 100, 20, [3, -3])], P0, N1, N)


def test_in_var_l1_bound(model16):
    """||Wr||_2^2 <= (2^(P0-1) / (2^n_e - 1))^2 for every query of either
    batch, and leveled_in_var is that bound times the fresh-LWE variance."""
    from fheicp.params import _tuniform_var
    from fheicp.stored import leveled_in_var
    c, _, queries, _ = model16
    bound2 = (2.0 ** (c.P0 - 1) / (2 ** c.cq.n_e - 1)) ** 2
    for idx in (list(range(8)), [q for q in range(8) if q != 5]):
        Wr, _, _, _ = c.plan_many(queries[idx], 0.5)
        for row in Wr:
            assert sum(int(x) ** 2 for x in row) <= bound2
            assert sum(abs(int(x)) for x in row) * (2 ** c.cq.n_e - 1) < 2 ** (c.P0 - 1)
    # a query concentrated on one feature comes close to the bound: more than
    # a quarter of it, where an all-features query stays below bound / D * 4
    one = np.zeros(16, np.float32)
    one[3] = -10.0
    Wr, _, _, P = c.plan_many(one[None, :], None)
    assert sum(int(x) ** 2 for x in Wr[0]) > bound2 / 4
    v = leveled_in_var(c.cq, c.P0, c.scheme)
    assert v == bound2 * _tuniform_var(c.scheme.glwe_noise_bits) / 2.0 ** 128
    # the packing plan made with it reaches the 9.2 sigma bar on this model
    from fheicp.params import pack_plan, pack_sigmas
    scheme = c.scheme.with_msg_bits(c.P0)
    b, L, lb = pack_plan(scheme, 1024, v)
    assert pack_sigmas(scheme, 1024, v, b, L, 63 - c.P0) >= 9.2 and 1 <= lb <= L
