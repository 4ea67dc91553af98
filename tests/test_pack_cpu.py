"""CPU: the LWE -> GLWE packing key switch and the evaluation-only context
 as far as they go without a device: key sizes, argument
checks on a host-only context, the gadget plan in C and in Python, and the
numpy restatement (tests/pack_ref.py) that the GPU tests compare against,
pinned here to the oracle's decompose_ks, negacyclic_mul and tuniform."""
import ctypes as C
import math

import numpy as np
import pytest

import pack_ref as R
from fheicp import _lib
from fheicp.params import TOY, pack_plan, pack_sigmas, params_for_bits

U = np.uint64


def host_ctx(p):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(_lib.params_struct(p.as_dict())), -1, C.byref(h)) == 0
    return L, h


def test_pack_key_words():
    L = _lib.lib()
    for p in (TOY, params_for_bits(16)):
        P = _lib.params_struct(p.as_dict())
        for beta, lv in ((4, 3), (7, 6), (6, 4), (1, 1), (6, 8)):
            assert L.fhe_pack_key_words(C.byref(P), beta, lv) == p.k * p.N * lv * (p.k + 1) * p.N
        for beta, lv in ((0, 3), (8, 3), (4, 0), (4, 9), (7, 8)):
            assert L.fhe_pack_key_words(C.byref(P), beta, lv) == 0


def test_pack_argument_checks_on_host_context():
    """Gadget and batch argument errors are FHE_E_ARG (-1) even on a host-only
    context, which reports everything else as FHE_E_DEVICE (-2)."""
    L, h = host_ctx(TOY)
    key = (C.c_uint32 * 8)(*range(8))
    buf = (C.c_uint64 * 8)()
    for beta, lv in ((0, 3), (8, 3), (4, 0), (4, 9), (7, 8)):      # 7 * 8 + 8 = 64 > 62
        assert L.fhe_keygen_pack_key(h, beta, lv, 1, None) == -1, (beta, lv)
        assert b"packing gadget" in L.fhe_last_error(h)
        assert L.fhe_keygen_pack_key_key(h, beta, lv, key, None) == -1
        assert L.fhe_import_pack_key(h, beta, lv, buf) == -1
    for ok in ((4, 3), (7, 7), (6, 8)):
        assert L.fhe_keygen_pack_key(h, ok[0], ok[1], 1, None) == -2
        assert L.fhe_import_pack_key(h, ok[0], ok[1], buf) == -2
    assert L.fhe_pack_batch(h, buf, -1, 0, buf, None) == -1
    assert L.fhe_pack_batch(h, buf, 4, -1, buf, None) == -1
    assert L.fhe_pack_batch(h, buf, 4, 9, buf, None) == -1
    assert b"pack" in L.fhe_last_error(h)
    assert L.fhe_pack_batch(h, buf, 4, 0, buf, None) == -2
    assert L.fhe_decrypt_packed_batch(h, buf, 4, 3, buf, None) == -1
    assert L.fhe_decrypt_packed_batch(h, buf, -1, 0, buf, None) == -1
    assert L.fhe_decrypt_packed_batch(h, buf, 4, 0, buf, None) == -2
    sq = L.fhe_search_query_batch
    assert sq(h, buf, 0, key, buf, 2, 0, buf, 0, 0, 0, buf, buf, None) == -1          # D = 0
    assert b"query" in L.fhe_last_error(h)
    assert sq(h, buf, 0, key, buf, -1, 4, buf, 0, 0, 0, buf, buf, None) == -1         # B < 0
    assert sq(h, buf, 0, key, buf, 2, 65537, buf, 0, 0, 0, buf, buf, None) == -1      # D too large
    assert sq(h, buf, 0, key, buf, 2, 4, buf, 0, 0, 9, buf, buf, None) == -1          # levels_bit > 8
    assert sq(h, buf, 0, key, buf, 2, 4, buf, 0, 0, 0, buf, buf, None) == -2
    assert L.fhe_import_eval_keys(h, buf, buf, None) == -2
    assert L.fhe_export_pack_key(h, buf) == -2
    nm = C.create_string_buffer(64)
    assert L.fhe_profile_kernel_name(h, b"pack", nm, 64) == 0 and nm.value == b""
    L.fhe_ctx_destroy(h)


@pytest.mark.parametrize("in_var", [0.0, (2.0 ** -33) ** 2])
def test_pack_plan_matches_library_and_rule(in_var):
    L = _lib.lib()
    for P in range(4, 28):
        p = params_for_bits(P)
        cp = _lib.params_struct(p.as_dict())
        for count in (1, 16, 1024):
            b, lv, lb = C.c_int32(), C.c_int32(), C.c_int32()
            assert L.fhe_pack_plan(C.byref(cp), count, in_var, C.byref(b), C.byref(lv), C.byref(lb)) == 0
            got = (b.value, lv.value, lb.value)
            assert got == pack_plan(p, count, in_var), (P, count)
            beta, lev, lbit = got
            assert 1 <= beta <= 7 and 1 <= lev <= 8 and beta * lev + lev <= 62 and 1 <= lbit <= lev

            def sigmas(be, le, mlog):      # the bar, from the model restated in pack_ref
                return 2.0 ** mlog / math.sqrt(in_var * 2.0 ** 128 + R.pack_var(p, count, be, le))
            assert sigmas(beta, lev, 63 - P) >= 9.2, (P, count, got)
            assert sigmas(beta, lev, 63 - P) == pack_sigmas(p, count, in_var, beta, lev, 63 - P)
            # fewest levels, then the largest base_log
            for le in range(1, lev + 1):
                for be in range(7, 0, -1):
                    if (le, -be) < (lev, -beta) and be * le + le <= 62:
                        assert sigmas(be, le, 63 - P) < 9.2, (P, count, got, be, le)
            assert sigmas(beta, lbit, 62) >= 9.2
            assert all(sigmas(beta, le, 62) < 9.2 for le in range(1, lbit))
    assert L.fhe_pack_plan(C.byref(cp), 0, 0.0, None, None, None) == -1
    assert L.fhe_pack_plan(C.byref(cp), 4, -1.0, None, None, None) == -1
    assert L.fhe_pack_plan(C.byref(cp), 4, 0.0, None, None, None) == 0


def test_restatement_helpers_match_oracle(oracle_lib):
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.integers(0, 2 ** 64, 400, dtype=U),
                         np.array([0, 2 ** 64 - 1, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 1 << 63, (1 << 63) - 1], U)])
    for beta, lv in ((4, 3), (7, 6), (6, 4), (3, 5), (7, 7), (1, 1), (6, 8)):
        # ties with both coins: the rounded value ends in B/2 at some level
        half = np.array([((1 << (beta - 1)) << (64 - beta * l)) | (c << (62 - beta * lv - (lv - l)))
                         for l in range(1, lv + 1) for c in (0, 1)], U)
        x = np.concatenate([xs, half])
        got = R.decompose_ks_np(x, beta, lv)
        for xi, gi in zip(x, got):
            np.testing.assert_array_equal(gi, oracle_lib.decompose_ks(int(xi), beta, lv))
        # the digits recompose x to within half the last level's weight
        with np.errstate(over="ignore"):
            rec = sum(got[:, l].astype(U) << U(64 - beta * (l + 1)) for l in range(lv))
            err = (x - rec).astype(np.int64)
        assert np.abs(err).max() <= 1 << (63 - beta * lv)
    w = rng.integers(0, 2 ** 64, 500, dtype=U)
    for b in (0, 17, 46):
        np.testing.assert_array_equal(R.tuniform_np(w, b), [oracle_lib.tuniform(int(x), b) for x in w])
    N = 256
    a, s = rng.integers(0, 2 ** 64, N, dtype=U), rng.integers(0, 2, N, dtype=U)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(a @ R.negacyclic_matrix(s, N), oracle_lib.negacyclic_mul(a, s))
    M = rng.integers(0, 2 ** 64, (3, 1, N), dtype=U)
    want = np.zeros(N, U)
    with np.errstate(over="ignore"):
        for j, jj in enumerate((0, 7, 255)):               # X^j as a polynomial factor
            mono = np.zeros(N, U)
            mono[jj] = 1
            want = oracle_lib.negacyclic_mul(mono, M[j, 0])
            rows = np.zeros((jj + 1, 1, N), U)
            rows[jj] = M[j]
            np.testing.assert_array_equal(R.rotate_sum(rows, np.zeros(jj + 1, U), N)[0], want)


def test_restatement_packs_and_decrypts_on_toy(oracle_lib):
    """300 TOY ciphertexts under the oracle's keys, a numpy-made packing key,
    two GLWEs: every message comes back exactly, and each packed phase is the
    input's phase plus an error within the model's 6 sigma."""
    p = TOY
    ref = oracle_lib.RefTFHE(p.as_dict(), seed=11)
    rng = np.random.default_rng(7)
    beta, lv, _ = pack_plan(p, 256, 0.0)
    pk = R.make_pack_key(rng, ref.s_big, p.N, p.k, beta, lv, p.glwe_noise_bits)
    assert pk.shape == (p.k * p.N, lv, p.k + 1, p.N)
    # the key rows decrypt to their messages with TUniform noise
    ph = R.glwe_phase(pk.reshape(-1, p.k + 1, p.N), ref.s_big, p.N, p.k).reshape(p.k * p.N, lv, p.N)
    with np.errstate(over="ignore"):
        for l in range(lv):
            ph[:, l, 0] -= ref.s_big << U(64 - beta * (l + 1))
    assert np.abs(ph.astype(np.int64)).max() <= 1 << p.glwe_noise_bits
    msgs = rng.integers(-(1 << (p.msg_bits - 1)), 1 << (p.msg_bits - 1), 300)
    msgs[:4] = (-(1 << (p.msg_bits - 1)), (1 << (p.msg_bits - 1)) - 1, 0, -1)
    ct = ref.encrypt_ints(msgs, seed=3)
    glwe = R.pack_ref(ct, pk, beta, lv)
    assert glwe.shape == (2, p.k + 1, p.N)
    phase = R.glwe_phase(glwe, ref.s_big, p.N, p.k).reshape(-1)[:300]
    err = (phase - ref.phase(ct)).astype(np.int64)
    sigma = math.sqrt(R.pack_var(p, 256, beta, lv))
    assert np.abs(err).max() <= 6 * sigma
    assert 0.8 * sigma <= err.std() <= 1.2 * sigma
    P = p.msg_bits
    q = ((phase >> U(63 - P)) + U(1)) >> U(1)
    q = (q & U((1 << P) - 1)).astype(np.int64)
    np.testing.assert_array_equal(np.where(q >= 1 << (P - 1), q - (1 << P), q), msgs)
    np.testing.assert_array_equal(ref.decrypt_ints(ct), msgs)
    # a level prefix packs too (coarser rounding): the first GLWE's slots past
    # count carry noise only
    few = R.pack_ref(ct[:17], pk, beta, 1)
    tail = R.glwe_phase(few, ref.s_big, p.N, p.k)[0, 17:].astype(np.int64)
    assert np.abs(tail).max() <= 6 * math.sqrt(R.pack_var(p, 17, beta, 1))
