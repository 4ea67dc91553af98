"""CPU: the both-private search as far as it goes without a
device: the numpy restatement (tests/extprod_ref.py) pinned to the oracle's
decompose_ks, negacyclic_mul and tuniform and decoded end to end at TOY size,
the gadget plan in C and in Python, argument checks on a host-only context and
the payload round trips of fheicp.private."""
import ctypes as C
import math

import numpy as np
import pytest

import extprod_ref as X
import pack_ref as R
from fheicp import _lib
from fheicp.params import TOY, extprod_plan, extprod_var, params_for_bits

U = np.uint64


def host_ctx(p):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(_lib.params_struct(p.as_dict())), -1, C.byref(h)) == 0
    return L, h


def test_restatement_pieces_match_oracle(oracle_lib):
    """query_poly, the GGSW messages and the Toeplitz operand against the
    oracle's negacyclic_mul; the level-major digits against decompose_ks; the
    rows' noise against tuniform."""
    rng = np.random.default_rng(3)
    N, k, beta, L = 64, 2, 5, 3
    W = np.array([7, -3, 0, 12, -128 * 31], np.int64)
    q = X.query_poly(W, N)
    # Q = sum_j W_j X^-j: multiplying a monomial X^p picks W_j at p - j
    mono = np.zeros(N, U)
    mono[9] = 1
    prod = oracle_lib.negacyclic_mul(mono, q).astype(np.int64)
    want = np.zeros(N, np.int64)
    want[9 - np.arange(5)] = W
    np.testing.assert_array_equal(prod, want)
    s_big = rng.integers(0, 2, k * N, dtype=U)
    msg = X.ggsw_messages(W, s_big, N, k, beta, L)
    with np.errstate(over="ignore"):
        for c in range(k + 1):
            m = q if c == k else U(0) - oracle_lib.negacyclic_mul(s_big[c * N:(c + 1) * N], q)
            for l in range(L):
                np.testing.assert_array_equal(msg[c, l], m << U(64 - beta * (l + 1)))
    ggsw = X.make_ggsw(rng.integers(0, 2 ** 64, ((k + 1) * L, k, N), dtype=U),
                       rng.integers(0, 2 ** 64, ((k + 1) * L, N), dtype=U), W, s_big, N, k, beta, L, 9)
    glwe = rng.integers(0, 2 ** 64, (2, k + 1, N), dtype=U)
    glwe[1, 0, :4] = (0, 2 ** 64 - 1, 0x8080808080808080, 1 << 63)
    out = X.external_product(glwe, ggsw, beta)
    with np.errstate(over="ignore"):
        for g in range(2):
            acc = np.zeros((k + 1, N), U)
            for c in range(k + 1):
                d = np.array([oracle_lib.decompose_ks(int(x), beta, L) for x in glwe[g, c]], np.int64)
                for l in range(L):
                    for cp in range(k + 1):
                        acc[cp] += oracle_lib.negacyclic_mul(d[:, l].astype(U), ggsw[c, l, cp])
            np.testing.assert_array_equal(out[g], acc)
    # the rows' phases are their messages plus the oracle's tuniform of the noise words
    nw = rng.integers(0, 2 ** 64, ((k + 1) * L, N), dtype=U)
    g2 = X.make_ggsw(rng.integers(0, 2 ** 64, ((k + 1) * L, k, N), dtype=U), nw, W, s_big, N, k, beta, L, 9)
    with np.errstate(over="ignore"):
        err = (R.glwe_phase(g2.reshape(-1, k + 1, N), s_big, N, k) - msg.reshape(-1, N)).astype(np.int64)
    np.testing.assert_array_equal(err[0, :50], [oracle_lib.tuniform(int(x), 9) for x in nw[0, :50]])
    # slot extraction: the LWE's phase is the GLWE's phase at the slot
    lwe = X.extract_slots(out, 5, 21, 0)                                # S = 3 slots per GLWE
    ph = R.glwe_phase(out, s_big, N, k)
    np.testing.assert_array_equal(X.lwe_phase(lwe, s_big), [ph[b // 3, (b % 3) * 21] for b in range(5)])


@pytest.mark.parametrize("D,same_sign", [(5, False), (16, False), (16, True)])
def test_restatement_decodes_clear_sum_on_toy(oracle_lib, D, same_sign):
    """Documents packed and encrypted by the oracle at TOY (N = 256, k = 2),
    a numpy-made GGSW on the planned gadget: every slot decodes to
    sum_j W_j dq[b, j] + cst. The error is checked against the model with its
    rounding term refined for the binary key: the rounding errors of two
    coefficients a slot sums share about half their variance (every mask
    coefficient meets a set key bit in both with probability 1/4, in one with
    1/2), so ||W||^2 (1 + kN/2) becomes ||W||^2 + (kN/4) (||W||^2 + (sum W)^2);
    same-sign weights are the worst case, up to sqrt((D + 1) / 2) model sigmas."""
    P = 12
    p = TOY.with_msg_bits(P)
    ref = oracle_lib.RefTFHE(p.as_dict(), seed=11)
    rng = np.random.default_rng(7 + D)
    S = p.N // D
    B = 7 * S + 3                                                       # eight GLWEs, the last partial
    dq = rng.integers(-4, 4, (B, D))
    W = rng.integers(-3, 4, D)
    W[0], W[D // 2] = -3, 0
    if same_sign:
        W = np.abs(W)
    cst = -17
    w2 = float(np.sum(W * W))
    beta, L = extprod_plan(p, 0.5 * (w2 + float(np.abs(W).sum()) ** 2))  # planned as fheicp.private does
    big = p.k * p.N
    refined = X.extprod_var(p, w2, beta, L) + 2.0 ** (2 * (64 - beta * L)) / 12.0 * (
        big / 4.0 * (w2 + float(W.sum()) ** 2) - big / 2.0 * w2)
    sigma = math.sqrt(refined)
    assert 2.0 ** (63 - P) / sigma >= 9.2
    glwe = ref.encrypt_packed(X.pack_docs_rows(dq, p.N), seed=5)[:, 0].reshape(-1, p.k + 1, p.N)
    assert len(glwe) == 8
    rows = (p.k + 1) * L
    ggsw = X.make_ggsw(rng.integers(0, 2 ** 64, (rows, p.k, p.N), dtype=U),
                       rng.integers(0, 2 ** 64, (rows, p.N), dtype=U), W, ref.s_big, p.N, p.k, beta, L,
                       p.glwe_noise_bits)
    lwe = X.linear_ggsw_ref(glwe, ggsw, beta, B, D, cst, P)
    assert lwe.shape == (B, p.k * p.N + 1)
    want = dq @ W + cst
    np.testing.assert_array_equal(ref.decrypt_ints(lwe), want)
    with np.errstate(over="ignore"):
        err = (ref.phase(lwe) - (want.astype(U) << U(64 - P))).astype(np.int64)
    print(f"D={D} same_sign={same_sign} gadget ({beta},{L}): sigma / refined {err.std() / sigma:.3f}, "
          f"/ model {err.std() / math.sqrt(X.extprod_var(p, w2, beta, L)):.3f}")
    assert np.abs(err).max() <= 6 * sigma
    # 100 to 400 slots whose errors share the GLWE's roundings: a wide band
    assert 0.7 * sigma <= err.std() <= 1.3 * sigma


def test_extprod_plan_matches_library_and_rule():
    L = _lib.lib()
    for P in range(8, 28):
        p = params_for_bits(P)
        cp = _lib.params_struct(p.as_dict())
        _, h = host_ctx(p)
        got_p = _lib.FheParams()
        assert L.fhe_get_params(h, C.byref(got_p)) == 0
        for w2 in (1.0, 4.0 ** 5 * 16 * 31 ** 2, 4.0 ** 7 * 768 * 127 ** 2, 2.0 ** 60):
            b, lv = C.c_int32(-1), C.c_int32(-1)
            rc = L.fhe_extprod_plan(C.byref(got_p), w2, C.byref(b), C.byref(lv))
            want = extprod_plan(p, w2)
            if want is None:
                assert rc == -3 and (b.value, lv.value) == (0, 0), (P, w2)
                assert b"9.2 sigma" in L.fhe_last_error(None)
                continue
            assert rc == 0 and (b.value, lv.value) == want, (P, w2)
            beta, lev = want
            assert 1 <= beta <= 7 and 1 <= lev <= 8 and lev * (beta + 1) <= 62

            def sigmas(be, le):                        # the bar, from the model restated in extprod_ref
                return 2.0 ** (63 - P) / math.sqrt(X.extprod_var(p, w2, be, le))
            assert sigmas(beta, lev) >= 9.2
            assert X.extprod_var(p, w2, beta, lev) == extprod_var(p, w2, beta, lev)
            for le in range(1, lev + 1):               # fewest levels, then the largest base_log
                for be in range(7, 0, -1):
                    if (le, -be) < (lev, -beta) and le * (be + 1) <= 62:
                        assert sigmas(be, le) < 9.2, (P, w2, want, be, le)
        L.fhe_ctx_destroy(h)
    assert extprod_plan(params_for_bits(27), 2.0 ** 60) is None
    assert L.fhe_extprod_plan(C.byref(cp), -1.0, None, None) == -1
    assert L.fhe_extprod_plan(C.byref(cp), 1.0, None, None) == 0
    with pytest.raises(ValueError):
        extprod_plan(TOY, -1.0)


def test_ggsw_sizes_and_argument_checks_on_host_context():
    """Argument errors are FHE_E_ARG (-1) even on a host-only context, which
    reports everything else, fhe_encrypt_ggsw included, as FHE_E_DEVICE (-2)."""
    L, h = host_ctx(TOY)
    P = _lib.params_struct(TOY.as_dict())
    k, N = TOY.k, TOY.N
    for beta, lv in ((4, 3), (7, 7), (1, 1), (6, 8)):
        assert L.fhe_ggsw_words(C.byref(P), beta, lv) == (k + 1) * lv * (k + 1) * N
    for beta, lv in ((0, 3), (8, 3), (4, 0), (4, 9), (7, 8)):
        assert L.fhe_ggsw_words(C.byref(P), beta, lv) == 0
    # S = N // D documents per GLWE, GLWEs padded to 16, one byte per word and level
    for B, D, lv, G in ((1, 1, 3, 1), (256, 1, 3, 1), (257, 1, 3, 2), (17, 16, 7, 2), (17, 256, 2, 17), (52, 5, 1, 2)):
        assert L.fhe_glwe_docs_bytes(C.byref(P), B, D, lv) == -(-G // 16) * 16 * (k + 1) * N * lv, (B, D)
    assert L.fhe_glwe_docs_bytes(C.byref(P), 4, 257, 3) == 0            # D > N
    assert L.fhe_glwe_docs_bytes(C.byref(P), 4, 0, 3) == 0
    assert L.fhe_glwe_docs_bytes(C.byref(P), 4, 4, 9) == 0
    key = (C.c_uint32 * 8)(*range(8))
    buf = (C.c_uint64 * 8)()
    assert L.fhe_encrypt_ggsw(h, buf, 4, 4, 3, 1, 0, buf, None) == -2
    assert b"host-only" in L.fhe_last_error(h)
    assert L.fhe_encrypt_ggsw_key(h, buf, 4, 4, 3, key, 0, buf, None) == -2
    assert L.fhe_encrypt_ggsw_key(h, buf, 4, 4, 3, None, 0, buf, None) == -1
    assert L.fhe_encrypt_ggsw(h, buf, 4, 8, 3, 1, 0, buf, None) == -1
    assert b"ggsw gadget" in L.fhe_last_error(h)
    assert L.fhe_encrypt_ggsw(h, buf, 257, 4, 3, 1, 0, buf, None) == -1
    assert b"D > N" in L.fhe_last_error(h)
    assert L.fhe_encrypt_ggsw(h, buf, 0, 4, 3, 1, 0, buf, None) == -1
    assert L.fhe_glwe_docs_pack(h, buf, 4, 257, 4, 3, buf, None) == -1
    assert L.fhe_glwe_docs_pack(h, buf, -1, 4, 4, 3, buf, None) == -1
    assert L.fhe_glwe_docs_pack(h, buf, 4, 4, 7, 8, buf, None) == -1
    assert L.fhe_glwe_docs_pack(h, buf, 4, 4, 4, 3, buf, None) == -2
    assert L.fhe_linear_ggsw_batch(h, buf, 4, 3, buf, 4, 257, 0, buf, None) == -1
    assert L.fhe_linear_ggsw_batch(h, buf, 4, 9, buf, 4, 4, 0, buf, None) == -1
    assert L.fhe_linear_ggsw_batch(h, buf, 4, 3, buf, 4, 4, 0, buf, None) == -2
    assert L.fhe_compare_ggsw_batch(h, buf, 4, 3, buf, -1, 4, 0, 0, buf, buf, None) == -1
    assert L.fhe_compare_ggsw_batch(h, buf, 4, 3, buf, 4, 4, 0, 0, buf, buf, None) == -2
    assert L.fhe_search_ggsw_batch(h, buf, 4, 3, buf, 4, 4, 0, 0, 9, buf, buf, None) == -1
    assert L.fhe_search_ggsw_batch(h, buf, 4, 3, buf, 4, 4, 0, 0, 0, buf, buf, None) == -2
    nm = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"linear_ggsw", nm, 64) == 0 and nm.value == b""
    L.fhe_ctx_destroy(h)


def test_payload_round_trips():
    from fheicp import private as PV
    rng = np.random.default_rng(1)
    N, k, beta, lv, D, P0 = 256, 2, 7, 6, 16, 21
    g = rng.integers(0, 2 ** 64, (k + 1) * lv * (k + 1) * N, dtype=U)
    pay = PV.pack_ggsw_query(g, D, P0, beta, lv, N, k)
    assert pay.dtype == U and pay.size == PV.HEADER_WORDS + g.size
    pl = PV.unpack_ggsw_query(pay)
    assert (pl["D"], pl["P0"], pl["base_log"], pl["level"], pl["N"], pl["k"]) == (D, P0, beta, lv, N, k)
    np.testing.assert_array_equal(pl["ggsw"], g)
    B = 37                                                              # S = 16 per GLWE: 3 GLWEs
    gl = rng.integers(0, 2 ** 64, 3 * (k + 1) * N, dtype=U)
    blk = PV.pack_doc_block(gl, B, D, P0, N, k)
    bl = PV.unpack_doc_block(blk)
    assert (bl["B"], bl["D"], bl["P0"], bl["N"], bl["k"]) == (B, D, P0, N, k)
    np.testing.assert_array_equal(bl["glwe"], gl)
    for bad in (pay[:-1], blk[:-1], pay.astype(np.int64), np.concatenate([blk[:1], pay[1:]])):
        with pytest.raises(ValueError):
            PV.unpack_ggsw_query(bad)
    for bad in (blk[:-1], pay, PV.pack_doc_block(gl, B, 257, P0, N, k)):
        with pytest.raises(ValueError):
            PV.unpack_doc_block(bad)
    v2 = pay.copy()
    v2[1] = 2
    with pytest.raises(ValueError, match="version"):
        PV.unpack_ggsw_query(v2)
    # the two payloads and the other modes' do not parse as each other
    from fheicp.query import unpack_query, unpack_reply
    for f in (unpack_query, unpack_reply):
        with pytest.raises(ValueError):
            f(pay)


def test_private_client_refuses_without_a_gadget():
    """plan_gadget reports a width no int8 gadget reaches (the digits stop at
    49 bits) instead of planning below the bar."""
    from types import SimpleNamespace
    from fheicp.private import plan_gadget, worst_norm2
    cq = SimpleNamespace(model=SimpleNamespace(q_w=np.full(768, 127)), n_e=8)
    # the correlated-rounding worst case: (sum q_w^2 + (sum |q_w|)^2) / 2 at |qq_j| = 2^(n_e - 1)
    assert worst_norm2(cq) == 4.0 ** 7 * 0.5 * (768 * 127 ** 2 + (768 * 127) ** 2)
    with pytest.raises(ValueError, match="no GGSW gadget at P0 = 27"):
        plan_gadget(params_for_bits(27), cq)
    small = SimpleNamespace(model=SimpleNamespace(q_w=np.full(16, 31)), n_e=6)
    assert plan_gadget(params_for_bits(21), small) == extprod_plan(params_for_bits(21), worst_norm2(small))
