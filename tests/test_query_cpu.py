"""CPU: the private-query mode (fheicp.query) — the query
payload, the BatchConfig rules, the new entry points' validation on a
host-only context, the planning against the oracle restatement, and the
balanced byte-plane split the GEMM's exactness rests on."""
import ctypes as C

import numpy as np
import pytest

from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.corpus import HEADER_WORDS, CorpusQuant, EncryptedCorpus, pack_payload
from fheicp.params import TOY, params_for_bits
from fheicp.query import MAGIC, EncryptedQuerySearch, pack_query, unpack_query


def test_query_payload_round_trip_and_rejection():
    key = np.arange(8, dtype=np.uint32) * 7919 + 3
    body = np.arange(16, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    pl = pack_query(body, 2 ** 63 + 9, 21, key, 2048)
    assert pl.dtype == np.uint64 and pl.size == HEADER_WORDS + 16 and int(pl[0]) == MAGIC
    u = unpack_query(pl)
    assert (u["D"], u["P0"], u["id0"], u["big"]) == (16, 21, 2 ** 63 + 9, 2048)
    np.testing.assert_array_equal(u["mask_key"], key)
    np.testing.assert_array_equal(u["body"], body)
    # a document payload is not a query payload (its own magic), nor is a
    # signed view or a truncated one
    for bad in (pack_payload(body, 1, 21, key, 2048), pl.astype(np.int64), pl[:-1], pl[:HEADER_WORDS - 1]):
        with pytest.raises(ValueError):
            unpack_query(bad)
    v2 = pl.copy()
    v2[1] = 2
    with pytest.raises(ValueError, match="version"):
        unpack_query(v2)


def test_batch_config_rules():
    from batch_operations import BatchConfig
    assert BatchConfig().encrypt_query is False
    assert BatchConfig(encrypt_query=True, fhe="execute").encrypt_query
    with pytest.raises(ValueError, match="store_ciphertexts"):
        BatchConfig(encrypt_query=True, store_ciphertexts=True, fhe="execute")
    for mode in ("simulate", "disable"):
        with pytest.raises(ValueError, match="execute"):
            BatchConfig(encrypt_query=True, fhe=mode)


def test_query_entry_points_on_host_context():
    L = _lib.lib()
    P = _lib.params_struct(params_for_bits(16).as_dict())
    # documented padding: B to a multiple of 16, D to a multiple of 64, one byte each
    for B, D, want in ((1, 1, 16 * 64), (16, 64, 16 * 64), (17, 65, 32 * 128), (1024, 16, 1024 * 64),
                       (1024, 768, 1024 * 768), (0, 16, 0)):
        assert L.fhe_query_docs_bytes(C.byref(P), B, D) == want, (B, D)
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(P), -1, C.byref(h)) == 0
    key = (C.c_uint32 * 8)()
    assert L.fhe_query_docs_pack(h, None, 4, 16, None, None) == -2
    assert b"host-only" in L.fhe_last_error(h)
    assert L.fhe_linear_query_batch(h, None, None, 4, 16, None, 0, None, None) == -2
    assert L.fhe_compare_query_batch(h, None, 0, key, None, 4, 16, None, 0, 0, None, None, None) == -2
    for D in (0, 65537):
        assert L.fhe_query_docs_pack(h, None, 4, D, None, None) == -1
        assert b"query" in L.fhe_last_error(h)
        assert L.fhe_linear_query_batch(h, None, None, 4, D, None, 0, None, None) == -1
        assert L.fhe_compare_query_batch(h, None, 0, key, None, 4, D, None, 0, 0, None, None, None) == -1
        assert b"query" in L.fhe_last_error(h)
    assert L.fhe_linear_query_batch(h, None, None, -1, 16, None, 0, None, None) == -1
    buf = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"linear_query", buf, 64) == 0 and buf.value == b""
    L.fhe_ctx_destroy(h)


@pytest.mark.parametrize("n_bits", [6, 8])
def test_planning_matches_oracle(n_bits):
    """P0 and T of EncryptedQuerySearch (pure numpy: the corpus object is
    never compiled) are the oracle's worst-case width and its threshold on the
    +-bound range; the weights are q_w unshifted."""
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    X, y = Q.prepare_training_data(16, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, n_bits)
    oq = Q.fit_quantized_linear(X, y, n_bits)
    e1, e2 = training_embeddings(16, 1000, seed=0)
    cq = CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2]))
    qs = EncryptedQuerySearch(EncryptedCorpus(cq))
    assert not qs.corpus.compiled
    assert qs.P0 == Q.corpus_worst_bits(oq, cq.s_e, n_bits)
    bound = int(np.abs(oq.q_w).sum()) * 4 ** (n_bits - 1) + abs(Q.corpus_qb(oq, cq.s_e))
    assert qs.bound() == bound

    class _Scale:   # Q.threshold_int reads only out_scale
        out_scale = Q.corpus_out_scale(oq, cq.s_e)
    for t in (0.5, 0.0, -0.25, 1e9, -1e9):
        w, cst, T = qs.plan(t)
        np.testing.assert_array_equal(w, oq.q_w)
        assert cst == Q.corpus_qb(oq, cq.s_e)
        assert T == Q.threshold_int(_Scale, t, -bound, bound)
        assert -bound <= T <= bound + 1
        # acc - T fits the P0-bit encoding for every reachable accumulator
        assert -(2 ** (qs.P0 - 1)) <= -bound - T and bound - T < 2 ** (qs.P0 - 1)
    assert qs.plan(None)[2] == -bound
    # the payload check refuses other parameters and a wrong width
    big = qs.corpus.scheme.k * qs.corpus.scheme.N
    key = np.zeros(8, np.uint32)
    qs.check(unpack_query(pack_query(np.zeros(16, np.uint64), 1, qs.P0, key, big)))
    for bad in (pack_query(np.zeros(16, np.uint64), 1, qs.P0 - 1, key, big),
                pack_query(np.zeros(16, np.uint64), 1, qs.P0, key, big // 2),
                pack_query(np.zeros(15, np.uint64), 1, qs.P0, key, big)):
        with pytest.raises(ValueError):
            qs.check(unpack_query(bad))


def test_pack_docs_refuses_wide_embeddings():
    from fheicp.model import FheLinearModel
    X, y = Q.prepare_training_data(16, 200, seed=5)
    m = FheLinearModel.fit(X, y, 6)
    qs = EncryptedQuerySearch(EncryptedCorpus(CorpusQuant(m.qparams, 9, 0.01), scheme=TOY))
    with pytest.raises(ValueError, match="n_e <= 8"):
        qs.pack_docs(np.zeros((2, 16), np.float32))


def byte_planes(x):
    """k_query_planes' split, restated: s_q = the low byte as a signed value,
    then (x - s_q) >> 8; eight planes, the last carry dropped."""
    x = np.asarray(x, dtype=np.uint64).copy()
    planes = []
    with np.errstate(over="ignore"):
        for _ in range(8):
            s = (x & np.uint64(0xff)).astype(np.uint8).view(np.int8)
            x = (x - s.astype(np.int64).view(np.uint64)) >> np.uint64(8)
            planes.append(s)
    return planes


def test_balanced_byte_planes_recombine():
    rng = np.random.default_rng(7)
    words = np.concatenate([rng.integers(0, 2 ** 64, 4096, dtype=np.uint64),
                            np.array([0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0, 1, 0x80,
                                      0x8000000000000000, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)])
    planes = byte_planes(words)
    assert all(p.dtype == np.int8 for p in planes)
    with np.errstate(over="ignore"):
        back = np.zeros_like(words)
        for q, s in enumerate(planes):
            back += s.astype(np.int64).view(np.uint64) << np.uint64(8 * q)
    np.testing.assert_array_equal(back, words)
    # and through a small integer GEMM, as the kernel's epilogue recombines it:
    # sum_q (dq @ s_q) << 8q == dq @ x modulo 2^64, with i32-sized partial sums
    dq = rng.integers(-128, 128, (5, words.size))
    dq[0], dq[1] = -128, 127
    with np.errstate(over="ignore"):
        want = (dq.astype(np.uint64) * words[None, :]).sum(1, dtype=np.uint64)
        got = np.zeros(5, np.uint64)
        for q, s in enumerate(planes):
            part = dq @ s.astype(np.int64)
            assert np.abs(part).max() <= words.size * 2 ** 14
            got += part.view(np.uint64) << np.uint64(8 * q)
    np.testing.assert_array_equal(got, want)
