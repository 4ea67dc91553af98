"""CPU: the noise-free rotation inputs of tests/rotation_ref.py against the
exact oracle, so the closed forms the GPU tests assert
(tests/test_gpu_rotation_exact.py) are not the helper's own opinion.

- trivial_expected equals the oracle's bootstrap for the three test-vector
  kinds (constant, staircase, table), at the toy set and at params_for_bits(16),
  on the classic rotation and on a multi-bit gadget;
- the one-hot case list has its stated length and reaches e in {-1, 0, +1},
  a1 = a2 = 0 with a12 = +-1 and sums that wrap past 2N (RefTFHE.modswitch),
  and exact_exponent agrees with the oracle's bootstrap of those rows;
- trivial big ciphertexts stay trivial through the oracle's key switch, sign
  extraction, bit extraction and threshold, with the sign body exactly 0 or
  2^63.
"""
from dataclasses import replace

import numpy as np
import pytest

import rotation_ref as R
from fheicp.params import TOY, params_for_bits

REAL16 = params_for_bits(16)
# the toy set with a multi-bit fast gadget (the real set's fast one is multi-bit already)
TOY_MB = replace(TOY, pbs_fast_base_log=8, pbs_fast_level=2, pbs_fast_group=2)
SETS = {"toy": TOY_MB, "real16": REAL16}


@pytest.fixture(scope="module")
def refs(oracle_lib):
    return {name: oracle_lib.RefTFHE(p.as_dict(), 99) for name, p in SETS.items()}


def table_lut(lut_bits: int) -> np.ndarray:
    """2^lut_bits distinct signed entries, lut[0] != 0."""
    m = np.arange(1 << lut_bits, dtype=np.int64)
    return (m * 37 + 11) % (1 << lut_bits) - (1 << (lut_bits - 1))


def test_switch_restates_the_oracle(refs):
    ref = refs["real16"]
    N, n = ref.N, ref.n
    rows = R.trivial_small(N, n)
    assert rows.shape == (3 * 2 * N, n + 1)
    got = R.switch(rows[:, n], N)
    assert np.array_equal(got, ref.modswitch(rows)[:, n].astype(np.int64))
    assert np.array_equal(got, R.trivial_exponents(N))
    assert got[-1] == 0 and got[-2] == 2 * N - 1      # the tie at j = 2N - 1 wraps


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("gadget", [0, 1])
def test_trivial_expected_vs_oracle(refs, name, gadget):
    ref = refs[name]
    prm = SETS[name]
    N, n, k, P = prm.N, prm.n, prm.k, prm.msg_bits
    assert (prm.pbs_fast_group if gadget else 1) == (2 if gadget else 1)
    rows = R.trivial_small(N, n)
    logN = N.bit_length() - 1
    for tv in (1 << 61, (1 << 61) + (1 << (64 - 16))):
        want = R.trivial_expected(rows, N, k, ("const", tv))
        assert np.array_equal(ref.pbs_gadget(rows, gadget, tv), want)
        if gadget == 0:
            assert np.array_equal(ref.pbs_const(rows, tv), want)
    lut = table_lut(logN - 1)
    assert len(set(lut.tolist())) == lut.size and lut[0] != 0
    want = R.trivial_expected(rows, N, k, ("table", lut, logN - 1, P))
    assert np.array_equal(ref.pbs_table(rows, lut, logN - 1, gadget=gadget), want)
    # every second exponent starts a new box: 2N / 2 boxes and the image of box 0
    assert len(set(want[:, -1].tolist())) >= N // 2
    if gadget == 0:
        for log_slots, step in ((logN, 1 << 48), (3, 1 << 50), (0, 0)):
            want = R.trivial_expected(rows, N, k, ("stairs", 1 << 61, step, log_slots))
            assert np.array_equal(ref.pbs_lut(rows, 1 << 61, step, log_slots), want)
            if log_slots == logN:
                assert len(set(want[:, -1].tolist())) == 2 * N      # every position distinct


@pytest.mark.parametrize("name", list(SETS))
def test_onehot_cases_reach_every_e(refs, name):
    ref = refs[name]
    prm = SETS[name]
    N, n = prm.N, prm.n
    rows, cases = R.onehot_small(N, n, ref.s_small, body=(N // 4 + 3) * R.unit(N))
    assert len(cases) == R.ONEHOT_CASES == 96 and rows.shape == (192, n + 1)
    sw = ref.modswitch(rows).astype(np.int64)
    assert np.array_equal(sw, R.switch(rows, N))
    assert np.array_equal(sw[1::2, n] - sw[0::2, n], np.ones(96, np.int64))
    es, a12s, wrapped = set(), set(), False
    for c, (idx, ws) in enumerate(cases):
        if len(idx) != 2:
            continue
        a1, a2 = sw[2 * c, idx[0]], sw[2 * c, idx[1]]
        pair = np.zeros((1, n + 1), np.uint64)
        with np.errstate(over="ignore"):
            pair[0, 0] = rows[2 * c, idx[0]] + rows[2 * c, idx[1]]
        a12 = int(ref.modswitch(pair)[0, 0])
        e = (a12 - a1 - a2) % (2 * N)
        e = e - 2 * N if e >= N else e
        assert e == R.pair_e(ws[0], ws[1], N)
        es.add(int(e))
        if a1 == 0 and a2 == 0:
            a12s.add(a12)
        wrapped |= (ws[0] & R.M64) + (ws[1] & R.M64) >= 1 << 64
    assert es == {-1, 0, 1}
    assert {1, 2 * N - 1} <= a12s          # a1 = a2 = 0 with a12 = +-1
    assert wrapped
    # the pair choice covers every key pattern
    s = ref.s_small.astype(np.int64)
    assert {(int(s[i[0]]), int(s[i[1]])) for i, _ in cases if len(i) == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the last single index is the lone last coefficient where n is odd
    assert (n - 1,) in {i for i, _ in cases}


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("gadget", [0, 1])
def test_exact_exponent_vs_oracle(refs, name, gadget):
    """The clear prediction of a one-hot row's table value (exact_exponent,
    then tv_at) equals the oracle's bootstrap, decoded; with body = None the
    two rows of a case straddle a constant test vector's sign flip."""
    ref = refs[name]
    prm = SETS[name]
    N, n, P = prm.N, prm.n, prm.msg_bits
    logN = N.bit_length() - 1
    group = 2 if gadget else 1
    lut = table_lut(logN - 1)
    rows, _ = R.onehot_small(N, n, ref.s_small, body=(N // 4 + 3) * R.unit(N), group=group)
    ex = R.exact_exponent(rows, ref.s_small, N, group)
    want = R.tv_at(("table", lut, logN - 1, P), ex, N)
    ph = ref.phase(ref.pbs_table(rows, lut, logN - 1, gadget=gadget))
    half = np.uint64(1 << (63 - P))
    assert np.array_equal((ph + half) >> np.uint64(64 - P), want >> np.uint64(64 - P))
    rows, _ = R.onehot_small(N, n, ref.s_small, body=None, group=group)
    ex = R.exact_exponent(rows, ref.s_small, N, group)
    assert np.array_equal(ex, np.tile([N - 1, N], 96))
    ph = ref.phase(ref.pbs_gadget(rows, gadget, 1 << 61)).view(np.int64)
    assert np.array_equal(ph > 0, np.tile([True, False], 96))


@pytest.mark.parametrize("name,P", [("toy", 8), ("toy", 5), ("real16", 16)])
def test_trivial_big_stays_trivial(oracle_lib, name, P):
    prm = replace(TOY if name == "toy" else REAL16, msg_bits=P)
    ref = oracle_lib.RefTFHE(prm.as_dict(), 99)
    N, k = prm.N, prm.k
    big = R.trivial_big(N, k, P, max_rows=512)
    small = ref.keyswitch(big)
    assert not small[:, :-1].any() and np.array_equal(small[:, -1], big[:, -1])
    # rounded: the +-2^(62-P) shifts stay a quarter step from the value
    v = (big[:, -1] + np.uint64(1 << (63 - P))).view(np.int64) >> (64 - P)
    sign, cv = R.oracle_sign_consuming(oracle_lib, ref, big)
    assert np.array_equal(sign, ref.sign_extract(big))
    assert not sign[:, :-1].any() and not cv[:, :-1].any()
    assert np.array_equal(sign[:, -1], np.where(v < 0, np.uint64(1 << 63), np.uint64(0)))
    refreshed, bsign, cv = R.oracle_bit_extract_consuming(oracle_lib, ref, big)
    assert not refreshed[:, :-1].any() and not bsign[:, :-1].any() and not cv[:, :-1].any()
    assert np.array_equal(bsign[:, -1], sign[:, -1])
    assert np.array_equal(refreshed[:, -1], v.astype(np.uint64) << np.uint64(64 - P))
    h = 1 << (P - 1)
    for T in (-h + 1, 0, h - 1):
        ok = (v - T >= -h) & (v - T < h)       # acc - T must fit msg_bits bits
        bit = ref.threshold(big[ok], T)
        assert not bit[:, :-1].any()
        assert np.array_equal(bit[:, -1], np.where(v[ok] >= T, np.uint64(1 << 63), np.uint64(0)))
