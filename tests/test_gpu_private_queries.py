"""GPU: the both-private search for several GGSW queries in one pass
 through libfheicp.

The batched leveled step (reversed document digits, GGSW byte planes, the
transposed i8 MFMA GEMM, slot extraction per query) word for word against the
single-query path and the numpy restatement (tests/extprod_ref.py); the
single-party compare against three single-query calls and the oracle's
restatement (quant_ref.corpus_*); the evaluation-only server's version-2
replies; the integration binding."""
import numpy as np
import pytest
import torch

import extprod_ref as X
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine, u64
from fheicp.params import TOY, extprod_plan

pytestmark = pytest.mark.gpu

U = np.uint64
GADGETS = [(4, 3), (7, 7)]
EDGE_WORDS = (0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0, 1 << 63)   # tests/test_gpu_extprod.py's
QMAX = 11
CSTS = [-37, 5, 0, 11, -1, 300, -4096, 2, 7, -8, 1]     # per query; negative ones among them


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(eng.device)


@pytest.fixture(scope="module")
def toy(need_gpu):
    eng = Engine(TOY, 0)
    eng.keygen(99)
    return eng


@pytest.fixture(scope="module")
def exact_ref(toy):
    """Per gadget: 11 GPU-made GGSWs (other weights and stream ids each) with
    the edge words planted in several of them, 17 document GLWEs of arbitrary
    words with the edge words and, on every level, the tie inputs with both
    coins, and the restatement's external product of all 17 under every query,
    computed once."""
    eng = toy
    p = eng.params
    out = {}
    for beta, L in GADGETS:
        rng = np.random.default_rng(200 * beta + L)
        ggsws = []
        for q in range(QMAX):
            W = rng.integers(-2 ** 12, 2 ** 12, 16)
            W[q % 16] = 0
            g = u64(eng.encrypt_ggsw(W, beta, L, 77 + q, id0=1000 * q)).reshape(p.k + 1, L, p.k + 1, p.N).copy()
            for i, w in enumerate(EDGE_WORDS):
                g[(i + q) % (p.k + 1), (i + q) % L, (i + 1) % (p.k + 1), 3 * i + q:3 * i + q + 2] = U(w)
            ggsws.append(g)
        ggsws = np.stack(ggsws)
        glwe = rng.integers(0, 2 ** 64, (17, p.k + 1, p.N), dtype=U)
        for i, w in enumerate(EDGE_WORDS):
            glwe[i % 17, i % (p.k + 1), 5 * i:5 * i + 3] = U(w)
        prec = beta * L
        ties = [((1 << (beta - 1)) << (64 - beta * l)) | (c << (62 - prec - (L - l))) for l in range(1, L + 1)
                for c in (0, 1)]
        for g in (0, 1, 16):                               # in every G of the cases below
            glwe[g, (g + p.k) % (p.k + 1), 40:40 + len(ties)] = np.array(ties, U)
        prod = np.stack([X.external_product(glwe, ggsws[q], beta) for q in range(QMAX)])
        out[(beta, L)] = (ggsws, glwe, prod)
    return out


def _shape(p, G, D):
    S = p.N // D
    B = G * S if S == 1 else (G - 1) * S + max(1, S // 3)   # the last GLWE partly filled
    return S, B


# Q in {1, 3, 6, 11}: (k+1) Q = 3, 9, 18, 33 rows, inside one 16-row tile, just
# past one, past two. G in {1, 2, 17}, D in {1, 5, 16, 256}, both gadgets:
# every value of each axis, the cross product sparsely.
CASES = [((4, 3), 1, 1, 1), ((4, 3), 3, 2, 5), ((4, 3), 6, 17, 16), ((4, 3), 11, 2, 256), ((4, 3), 3, 17, 1),
         ((7, 7), 1, 17, 256), ((7, 7), 3, 1, 16), ((7, 7), 6, 2, 1), ((7, 7), 11, 17, 5), ((7, 7), 6, 1, 256)]


@pytest.mark.parametrize("gadget,Qn,G,D", CASES)
def test_linear_ggsws_bit_exact(toy, exact_ref, gadget, Qn, G, D):
    """Rows [q B, (q + 1) B) of fhe_linear_ggsws_batch equal fhe_linear_ggsw_batch
    of query q and the restatement, word for word. The Q scaled constants sit
    in the workspace right after the result's last GLWE and are read after the
    GEMM, so a store past the result would show in the bodies."""
    eng = toy
    p = eng.params
    beta, L = gadget
    ggsws, glwe, prod = exact_ref[gadget]
    S, B = _shape(p, G, D)
    assert eng.doc_glwes(B, D) == G
    gl = dev_u64(eng, glwe[:G])
    docs = eng.pack_docs_glwe_queries(gl, B, D, beta, L)
    assert docs.numel() == G * (p.k + 1) * L * (2 * p.N + 16)
    csts = CSTS[:Qn]
    eng.profile(True)
    got = u64(eng.linear_ggsws(dev_u64(eng, ggsws[:Qn]), beta, L, docs, B, D, csts)).reshape(Qn, B, -1)
    eng.profile(False)
    assert eng.kernel_name("linear_ggsws") == f"k_extprod_queries_mfma<{1 if 3 * Qn <= 16 else 2}>"
    assert eng.profile_read("linear_ggsws")["items"] == Qn * B
    docs8 = eng.pack_docs_glwe(gl, B, D, beta, L)
    for q in range(Qn):
        want = X.extract_slots(prod[q][:G], B, D, (csts[q] << (64 - p.msg_bits)) % 2 ** 64)
        np.testing.assert_array_equal(got[q], want, err_msg=f"query {q} against the restatement")
        one = u64(eng.linear_ggsw(dev_u64(eng, ggsws[q]), beta, L, docs8, B, D, csts[q]))
        np.testing.assert_array_equal(got[q], one, err_msg=f"query {q} against linear_ggsw")


def test_linear_ggsws_canary(toy, exact_ref):
    """Q = 3, B = 68 (no multiple of 16): 16 sentinel rows after row Q B are
    untouched. The result workspace is context-owned; its tail is guarded by
    the Q constants stored right after its last GLWE and read after the GEMM
    (test_linear_ggsws_bit_exact)."""
    eng = toy
    p = eng.params
    beta, L = 7, 7
    ggsws, glwe, prod = exact_ref[(beta, L)]
    Qn, G, D = 3, 2, 5
    S, B = _shape(p, G, D)
    assert B % 16 and (Qn * B) % 16
    Wb = p.k * p.N + 1
    SENT = -0x0123456789ABCDEF
    buf = torch.full(((Qn * B + 16), Wb), SENT, dtype=torch.int64, device=eng.device)
    docs = eng.pack_docs_glwe_queries(dev_u64(eng, glwe[:G]), B, D, beta, L)
    out = eng.linear_ggsws(dev_u64(eng, ggsws[:Qn]), beta, L, docs, B, D, CSTS[:Qn], out=buf)
    assert out.data_ptr() == buf.data_ptr()
    got = u64(buf)
    assert (buf[Qn * B:] == SENT).all()
    for q in range(Qn):
        want = X.extract_slots(prod[q][:G], B, D, (CSTS[q] << (64 - p.msg_bits)) % 2 ** 64)
        np.testing.assert_array_equal(got[q * B:(q + 1) * B], want)


@pytest.fixture(scope="module")
def private16(need_gpu):
    """The 16-dim, n_bits 6 model of tests/test_gpu_extprod.py; the packing key
    planned for 3 x 64 results in one GLWE."""
    from fheicp.corpus import CorpusQuant, EncryptedCorpus
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    from fheicp.private import PrivateClient
    Xt, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(Xt, y, 6)
    oq = Q.fit_quantized_linear(Xt, y, 6)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client = PrivateClient(c, count=256, pack_seed=4, enc_seed=12)
    return c, client, oq, {}


def test_compare_ggsws_matches_single_queries(private16):
    """fhe_compare_ggsws_batch returns the (acc, below) of three
    fhe_compare_ggsw_batch calls and of quant_ref.corpus_*: Q = 3, B = 64,
    per-query thresholds, one the median score (bits on both sides)."""
    from fheicp.private import unpack_doc_block, unpack_ggsw_query
    c, client, oq, memo = private16
    eng = c.engine
    s_e = c.cq.s_e
    q0, docs = Q.make_corpus(16, 64, seed=21)
    queries = np.stack([q0, Q.make_corpus(16, 64, seed=31)[0], Q.make_corpus(16, 64, seed=32)[0]])
    ref_acc = np.stack([Q.corpus_accumulate(oq, s_e, 6, q, docs) for q in queries])
    scores = np.float64(Q.corpus_out_scale(oq, s_e)) * ref_acc.astype(np.float64)
    ts = [0.5, float(np.median(scores[1])), None]
    want = np.stack([(scores[q] < ts[q]).astype(np.int64) if ts[q] is not None else np.zeros(64, np.int64)
                     for q in range(3)])
    assert 0.25 <= want[1].mean() <= 0.75
    block = client.encrypt_docs(docs)
    payloads = client.encrypt_queries(queries, id0=2 ** 64 - 40)       # the id ranges cross the wrap
    pls = [unpack_ggsw_query(p) for p in payloads]
    bl = unpack_doc_block(block)
    gl = eng.to_dev(bl["glwe"])
    docsq = eng.pack_docs_glwe_queries(gl, 64, 16, *client.gadget)
    docs8 = eng.pack_docs_glwe(gl, 64, 16, *client.gadget)
    from fheicp.query import EncryptedQuerySearch
    _, cst, Ts = EncryptedQuerySearch(c).plan_many(ts, 3)
    eng.set_msg_bits(c.P0)
    ggsws = eng.to_dev(np.concatenate([pl["ggsw"] for pl in pls]))
    acc, below = eng.compare_ggsws(ggsws, *client.gadget, docsq, 64, 16, cst, Ts)
    assert acc.shape == below.shape == (3, 64)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref_acc)
    np.testing.assert_array_equal(below.cpu().numpy(), want)
    for q in range(3):
        a1, b1 = eng.compare_ggsw(eng.to_dev(pls[q]["ggsw"]), *client.gadget, docs8, 64, 16, cst, Ts[q])
        np.testing.assert_array_equal(acc[q].cpu().numpy(), a1.cpu().numpy())
        np.testing.assert_array_equal(below[q].cpu().numpy(), b1.cpu().numpy())
    memo.update(block=block, payloads=payloads, acc=ref_acc, below=want, ts=ts)


def test_search_many_on_evaluation_only_server(private16):
    """A server with evaluation keys only: the version-2 replies decrypt to the
    compare's values; compare_ggsws there is FHE_E_STATE; a gadget mismatch
    and a mixed batch raise."""
    from fheicp.private import PrivateServer, pack_ggsw_query, unpack_ggsw_query
    from fheicp.query import unpack_replies
    c, client, oq, memo = private16
    if not memo:
        test_compare_ggsws_matches_single_queries(private16)
    server = PrivateServer(client.eval_keys(), c.cq, c.P0, device=0, scheme=c.scheme)
    assert (server.base_log, server.level) == client.gadget
    docs, B = server.pack_docs_many(memo["block"])
    assert B == 64
    replies = server.search_many(memo["payloads"], docs, B, memo["ts"])
    assert isinstance(replies, list) and len(replies) == 1
    n1 = (c.scheme.k + 1) * c.scheme.N
    r = unpack_replies(replies[0], n1, c.scheme.N)
    assert (r["Q"], r["B"], r["P0"]) == (3, 64, c.P0)
    acc, below = client.decrypt_replies(replies)
    np.testing.assert_array_equal(acc.cpu().numpy(), memo["acc"])
    np.testing.assert_array_equal(below.cpu().numpy(), memo["below"])
    # one threshold for all, and the single-query reply of query 1 holds the same values
    rep1 = server.search_many(memo["payloads"], docs, B, memo["ts"][1])
    acc1, below1 = client.decrypt_replies(rep1)
    np.testing.assert_array_equal(acc1.cpu().numpy(), memo["acc"])
    np.testing.assert_array_equal(below1[1].cpu().numpy(), memo["below"][1])
    eng = server.engine
    with pytest.raises(_lib.FheError, match="FHE_E_STATE"):
        eng.compare_ggsws(eng.to_dev(np.zeros(3 * eng.ggsw_words(*client.gadget), np.int64)), *client.gadget, docs, B,
                          16, 0, [0, 0, 0])
    pl = unpack_ggsw_query(memo["payloads"][0])
    other = (pl["base_log"] - 1, pl["level"])
    words = (pl["k"] + 1) * other[1] * (pl["k"] + 1) * pl["N"]
    odd = pack_ggsw_query(np.zeros(words, U), pl["D"], pl["P0"], *other, pl["N"], pl["k"])
    with pytest.raises(ValueError, match="query 0: gadget"):
        server.search_many([odd, odd], docs, B, None)
    with pytest.raises(ValueError, match="query 2: gadget base_log"):
        server.search_many([memo["payloads"][0], memo["payloads"][1], odd], docs, B, None)
    with pytest.raises(ValueError, match="2 thresholds for 3"):
        server.search_many(memo["payloads"], docs, B, [0.5, 0.5])
    eng.close()


def test_integration_binding_ggsws(need_gpu):
    """integration/fhe_gpu.py's batched both-private calls (numpy and ctypes
    only) on TOY at 12 bits with planned gadgets: compare_ggsws returns the
    clear sums and bits per query, and search_ggsws' packed GLWEs decrypt to
    the same."""
    import sys
    from pathlib import Path
    from fheicp import LIB_PATH
    from fheicp.params import extprod_var
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "integration"))
    from fhe_gpu import GpuCompare
    p = TOY.with_msg_bits(12)
    eng = GpuCompare(p.as_dict(), key_seed=31, lib_path=str(LIB_PATH), enc_seed=1)
    try:
        rng = np.random.default_rng(9)
        Qn, B, D = 3, 70, 5                               # S = 51 per GLWE: two GLWEs
        dq, W = rng.integers(-8, 8, (B, D)), rng.integers(-9, 10, (Qn, D))
        cst, Ts = 11, [-20, 0, 35]
        want = dq @ W.T + cst                             # |acc - T| <= 5 * 8 * 9 + 46 < 2^11
        w2 = max(0.5 * (float(np.sum(w * w)) + float(np.abs(w).sum()) ** 2) for w in W)
        beta, L = eng.ggsw_plan(w2)
        assert (beta, L) == extprod_plan(p, w2)
        _, _, lb = eng.keygen_pack(count=Qn * B, in_var=extprod_var(p, w2, beta, L) / 2.0 ** 128, seed=32)
        glwe = eng.encrypt_docs_glwe(dq)
        ggsws = np.stack([eng.encrypt_ggsw(w, beta, L) for w in W])
        docs = eng.pack_docs_glwe_queries(glwe, B, D, beta, L)
        acc1, below1 = eng.compare_ggsws(ggsws, beta, L, docs, cst, Ts)
        ga, gb = eng.search_ggsws(ggsws, beta, L, docs, cst, Ts, lb)
        acc = eng.decrypt_packed(ga, Qn * B, 0).reshape(Qn, B) + np.array(Ts)[:, None]
        below = eng.decrypt_packed(gb, Qn * B, 1).reshape(Qn, B)
        eng.free_docs(docs)
    finally:
        eng.close()
    np.testing.assert_array_equal(acc1, want.T)
    np.testing.assert_array_equal(acc, want.T)
    np.testing.assert_array_equal(below, (want.T < np.array(Ts)[:, None]).astype(np.int64))
    np.testing.assert_array_equal(below1, below)
    assert all(0 < below[q].sum() < B for q in range(Qn))
