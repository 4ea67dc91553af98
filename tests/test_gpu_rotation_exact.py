"""GPU: the blind rotation word for word, on inputs that carry no noise.

Every other rotation test feeds the kernels key-switched random encryptions
and can only check statistics (tests/test_gpu_noise.py) or decrypted bits.
A small LWE with a zero mask meets no key: the classic kernels decompose
X^0 ACC - ACC = 0 and the multi-bit ones multiply by psi^0 - 1 = 0, so the
output is fixed by the body alone and must equal the closed form of
tests/rotation_ref.py and the oracle in every word (np.array_equal on whole
ciphertexts). That pins down what noise hides: the modulus switch of the body
at all 2N exponents and their ties, the initial rotation of each test-vector
kind with its negacyclic flip, sample extraction, the 32/48/64-bit accumulator
forms, the `c < count` guards, the isolation of the four ciphertexts of a
key-stationary workgroup, and the sign extraction's plumbing (shifts, add_body,
per-round test vectors, the ct_v / refreshed / sign epilogues), per kernel
instance the parameter table can select.

Masks with one or two nonzero words (rotation_ref.onehot_small) run one or two
external products: they put the exponent logic (a in {1, N-1, N, N+1, 2N-1},
the wrap to 0, the first and last index, the multi-bit a12 with e = -1, 0, +1)
on chosen values; the decoded output must equal the oracle's and the clear
prediction, the phase stays within the 8 sigma of a whole bootstrap.

Measured on MI355X, |phase - oracle's| over the one-hot rows in units of
sigma_model * sqrt(active steps / all steps), max (rms); printed by
test_onehot_vs_oracle and asserted only against the 8 sigma_model bound:
  v4 (15,2), constant      1.38 (0.51)    mw (15,2), table    1.93 (0.55)
  v4s (12,3), constant     2.44 (0.86)    mb (15,2), table    3.67 (0.97)
  mb64 (12,3), table       0.90 (0.19)    mb (23,1), table    0.005 (0.002)
At most 0.18 sigma_model in absolute terms. GPU and oracle share key and input
here, so the difference is what they do not share: the f64 FFT's arithmetic
error and the 2^32 output rounding of the 32-bit accumulators, both of which
the model charges per step at about the size of a step's key noise for the
level-2 and level-3 gadgets; (23,1)'s step is all gadget rounding, which both
sides round alike.
"""
import ctypes as C
import math
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rotation_ref as R
from test_gpu_noise import INSTANCES
from fheicp.engine import Engine, EngineGroup, _ptr, _stream, group_rows, u64
from fheicp.params import TOY, SchemeParams, _variances, params_for_bits

pytestmark = pytest.mark.gpu

TV = 1 << 61
TV_LOW = (1 << 61) + (1 << (64 - 16))     # low bits still inside the 32-bit accumulators' range
STEP = 1 << 48
PATTERN = 0x5A5A5A5A5A5A5A5A
SIGN_ROWS = 700      # values per shift of the real-parameter sign tests (three shifts: past 2048 rows)
REAL16 = params_for_bits(16)
MW = "k_blind_rotate_mw<fhei::V2, 2, 2, {}>"
EXTRA = {"toy": "k_blind_rotate<7, 2, BrTv>", "variant2": MW.format("BrTv")}


def table_lut(lut_bits: int) -> np.ndarray:
    """2^lut_bits distinct signed entries, lut[0] != 0."""
    m = np.arange(1 << lut_bits, dtype=np.int64)
    return (m * 37 + 11) % (1 << lut_bits) - (1 << (lut_bits - 1))


def instance_params(key):
    """(SchemeParams, gadget index, group, kernel name) of an entry of
    test_gpu_noise's instance table, built as that test builds it; "toy" (the
    one-wave kernel) and "variant2" (FHEICP_BR_VARIANT=2 at real parameters)."""
    if key == "toy":
        return TOY, 0, 1, EXTRA[key]
    if key == "variant2":
        return REAL16, 0, 1, EXTRA[key]
    beta, lvl, grp = key
    if grp == 1:
        return SchemeParams(pbs_base_log=beta, pbs_level=lvl, msg_bits=16), 0, 1, INSTANCES[key]
    prm = SchemeParams(msg_bits=16, pbs_fast_base_log=beta, pbs_fast_level=lvl, pbs_fast_group=2)
    return prm, 1, 2, INSTANCES[key]


def table_kernel(inst) -> str:
    if inst.group == 2:
        assert inst.name.endswith("BrTv>")
        return inst.name[:-len("BrTv>")] + "BrTvLut>"
    return "k_blind_rotate<7, 2, BrTvLut>" if inst.key == "toy" else MW.format("BrTvLut")


def make_instance(key, oracle_lib, seed=None):
    prm, g, grp, name = instance_params(key)
    with pytest.MonkeyPatch.context() as mp:
        if key == "variant2":
            mp.setenv("FHEICP_BR_VARIANT", "2")      # read when the context is created
        eng = Engine(prm, 0)
    if seed is None:
        seed = 5000 + (10 * key[0] + key[1] + 100 * (key[2] - 1) if isinstance(key, tuple) else 7)
    eng.keygen(seed)
    N, n, k = prm.N, prm.n, prm.k
    sweep = R.trivial_small(N, n)
    return SimpleNamespace(key=key, prm=prm, g=g, group=grp, name=name, eng=eng, seed=seed, N=N, n=n, k=k,
                           logN=N.bit_length() - 1, bucket="blind_rotate_main" if g == 0 else "blind_rotate_fast",
                           sweep=sweep, sweep_dev=eng.to_dev(sweep), full={},
                           ref0=R.keyless_oracle(oracle_lib, prm.as_dict()))


def _id(key):
    return key if isinstance(key, str) else "-".join(str(x) for x in key)


@pytest.fixture(scope="module", params=list(INSTANCES) + list(EXTRA), ids=_id)
def inst(request, need_gpu, oracle_lib):
    """One engine with keys per kernel instance, shared by the tests below
    (pytest groups the tests of a module-scoped parameter, so one lives at a
    time). The oracle beside it is keyless: its inputs have zero masks."""
    it = make_instance(request.param, oracle_lib)
    yield it
    it.eng.close()


def full_const(inst, tv):
    """The whole sweep through the constant test vector (run once per instance and tv)."""
    if ("const", tv) not in inst.full:
        inst.full["const", tv] = u64(inst.eng.pbs_gadget(inst.sweep_dev, inst.g, tv))
        assert inst.eng.kernel_name(inst.bucket) == inst.name
    return inst.full["const", tv]


def full_table(inst):
    """The whole sweep through the table test vector: on a multi-bit gadget
    its own kernel's BrTvLut instantiation, on gadget 0 the v2 / v1 kernel's."""
    if "table" not in inst.full:
        lut = table_lut(inst.logN - 1)
        inst.full["table"] = u64(inst.eng.pbs_table(inst.sweep_dev, lut, inst.logN - 1, gadget=inst.g))
        assert inst.eng.kernel_name(inst.bucket) == table_kernel(inst)
    return inst.full["table"]


# ------------------------------------------------------- a. per instance --
@pytest.mark.parametrize("tv", [TV, TV_LOW], ids=["tv61", "tv61+48"])
def test_trivial_sweep_constant(inst, tv):
    """All 2N exponents and their ties through the constant test vector:
    zero mask, body +-tv, every word."""
    got = full_const(inst, tv)
    want = R.trivial_expected(inst.sweep, inst.N, inst.k, ("const", tv))
    assert got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got, inst.ref0.pbs_gadget(inst.sweep, inst.g, tv))


def test_trivial_sweep_table_and_staircase(inst):
    """The table test vector (BrTvLut) with 2-wide boxes and distinct signed
    entries: an exponent off by one, a missed negacyclic flip or a shifted
    initial rotation changes a body. On gadget 0 also the staircase
    (fhe_pbs_lut_batch runs on the main gadget) with one slot per coefficient
    and a nonzero step: each of the 2N positions has its own value."""
    lut = table_lut(inst.logN - 1)
    P = inst.prm.msg_bits
    got = full_table(inst)
    want = R.trivial_expected(inst.sweep, inst.N, inst.k, ("table", lut, inst.logN - 1, P))
    assert np.array_equal(got, want)
    assert np.array_equal(got, inst.ref0.pbs_table(inst.sweep, lut, inst.logN - 1, gadget=inst.g))
    if inst.g == 0:
        got = u64(inst.eng.pbs_lut(inst.sweep_dev, TV, STEP, inst.logN))
        assert inst.eng.kernel_name(inst.bucket) == inst.name
        want = R.trivial_expected(inst.sweep, inst.N, inst.k, ("stairs", TV, STEP, inst.logN))
        assert len(set(want[:, -1].tolist())) == 2 * inst.N
        assert np.array_equal(got, want)
        assert np.array_equal(got, inst.ref0.pbs_lut(inst.sweep, TV, STEP, inst.logN))


# ------------------------------------------- b. ragged counts, the guard --
@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_ragged_counts_and_guard(inst, c):
    """The first c rows alone (a workgroup of four partly empty), into a
    buffer four rows longer and pre-filled: rows < c equal the full run's,
    rows >= c keep the pattern (an in-bounds check)."""
    eng = inst.eng
    small = inst.sweep_dev[:c].contiguous()
    full = full_const(inst, TV)
    buf = torch.full((c + 4, eng.W), PATTERN, dtype=torch.int64, device=eng.device)
    eng._chk(eng._L.fhe_pbs_gadget_batch(eng._ctx, _ptr(small), c, inst.g, C.c_uint64(TV), _ptr(buf),
                                         _stream(eng.device)))
    assert eng.kernel_name(inst.bucket) == inst.name
    got = u64(buf)
    assert np.array_equal(got[:c], full[:c])
    assert np.array_equal(got[c:], np.full((4, eng.W), PATTERN, np.uint64))
    full = full_table(inst)
    lut_d = eng.to_dev(table_lut(inst.logN - 1))
    buf = torch.full((c + 4, eng.W), PATTERN, dtype=torch.int64, device=eng.device)
    eng._chk(eng._L.fhe_pbs_table_gadget_batch(eng._ctx, _ptr(small), c, inst.g, _ptr(lut_d), inst.logN - 1,
                                               _ptr(buf), _stream(eng.device)))
    assert eng.kernel_name(inst.bucket) == table_kernel(inst)
    got = u64(buf)
    assert np.array_equal(got[:c], full[:c])
    assert np.array_equal(got[c:], np.full((4, eng.W), PATTERN, np.uint64))


# ------------------------------------------------------- c. neighbours --
@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_trivial_row_among_ordinary_rows(inst, slot):
    """64 rows, row 4 w + slot trivial and the other three of each workgroup
    ordinary key-switched encryptions: the trivial rows stay exact in every
    word, the ordinary ones decrypt to the sign of their message."""
    eng = inst.eng
    P = inst.prm.msg_bits
    sgn = np.where(np.arange(64) % 2 == 0, 1, -1).astype(np.int64)
    batch = eng.keyswitch(eng.encrypt(sgn * (1 << (P - 2)), seed=17 + slot), 0, 0).clone()
    pick = (np.arange(16) * 409 + 3 * slot + 2) % inst.sweep.shape[0]
    pick[-1] = inst.sweep.shape[0] - 1               # the tie that wraps to exponent 0
    triv = 4 * np.arange(16) + slot
    batch[torch.from_numpy(triv).to(eng.device)] = inst.sweep_dev[torch.from_numpy(pick).to(eng.device)]
    out_dev = eng.pbs_gadget(batch, inst.g, TV)
    assert eng.kernel_name(inst.bucket) == inst.name
    out = u64(out_dev)
    assert np.array_equal(out[triv], R.trivial_expected(inst.sweep[pick], inst.N, inst.k, ("const", TV)))
    rest = np.setdiff1d(np.arange(64), triv)
    ph = u64(eng.phase(out_dev)).view(np.int64)
    assert np.array_equal(ph[rest] > 0, sgn[rest] > 0)
    assert out[rest, :-1].any(axis=1).all()          # and they are real bootstraps: a mask


# ------------------------------------------------ d. one- and two-hot --
ONEHOT = {
    # key: (instance key, parameters, gadget, group, (base_log, level), table?)
    "v4-15-2": ((15, 2, 1), REAL16, 0, 1, (15, 2), False),
    "mw-table-15-2": ((15, 2, 1), REAL16, 0, 1, (15, 2), True),
    "mb-15-2": ((15, 2, 2), REAL16, 1, 2, (15, 2), True),
    "mb-23-1": ((23, 1, 2), REAL16, 2, 2, (23, 1), True),
    "mb64-12-3": ((12, 3, 2), instance_params((12, 3, 2))[0], 1, 2, (12, 3), True),
    "v4s-12-3": ((12, 3, 1), instance_params((12, 3, 1))[0], 0, 1, (12, 3), False),
}
BUCKETS = {0: "blind_rotate_main", 1: "blind_rotate_fast", 2: "blind_rotate_fast2"}


@pytest.fixture(scope="module")
def keyed(need_gpu, oracle_lib):
    """Engines and oracles on the same keys, by parameter set, made on demand."""
    made = {}

    def get(prm):
        if prm not in made:
            eng = Engine(prm, 0)
            eng.keygen(4242)
            made[prm] = (eng, oracle_lib.RefTFHE(prm.as_dict(), 4242))
        return made[prm]
    yield get
    for eng, _ in made.values():
        eng.close()


@pytest.mark.parametrize("case", list(ONEHOT))
def test_onehot_vs_oracle(keyed, case):
    """96 one- and two-hot masks at two bodies each (192 rows, all kept): the
    decoded output equals the oracle's and the clear prediction from s_small
    and the switched exponents; phases within 8 sigma_model of the oracle's;
    rows none of whose steps is active are exact in every word. The table
    bootstrap where the instance has one (2-wide boxes), else the constant
    test vector with the two bodies either side of its sign flip."""
    ikey, prm, g, grp, (beta, lvl), table = ONEHOT[case]
    eng, ref = keyed(prm)
    N, n, P = prm.N, prm.n, prm.msg_bits
    logN = N.bit_length() - 1
    s_small = eng.export_keys()["s_small"]
    assert np.array_equal(s_small, ref.s_small)
    if table:
        lut = table_lut(logN - 1)
        kind = ("table", lut, logN - 1, P)
        rows, cases = R.onehot_small(N, n, s_small, body=(N // 4 + 3) * R.unit(N), group=grp)
        out_dev = eng.pbs_table(eng.to_dev(rows), lut, logN - 1, gadget=g)
        name = INSTANCES[ikey][:-len("BrTv>")] + "BrTvLut>" if grp == 2 else MW.format("BrTvLut")
        out_ref = ref.pbs_table(rows, lut, logN - 1, gadget=g)
    else:
        kind = ("const", TV)
        rows, cases = R.onehot_small(N, n, s_small, body=None, group=grp)
        out_dev = eng.pbs_gadget(eng.to_dev(rows), g, TV)
        name = INSTANCES[ikey]
        out_ref = ref.pbs_gadget(rows, g, TV)
    assert eng.kernel_name(BUCKETS[g]) == name
    assert len(cases) == R.ONEHOT_CASES and rows.shape[0] == 192
    out = u64(out_dev)
    ph = u64(eng.phase(out_dev))
    ph_ref = ref.phase(out_ref)
    half, sh = np.uint64(1 << (63 - P)), np.uint64(64 - P)
    want = R.tv_at(kind, R.exact_exponent(rows, s_small, N, grp), N)
    dec = (ph + half) >> sh
    d = (ph - ph_ref).view(np.int64).astype(np.float64) / 2.0 ** 64
    sigma_model = math.sqrt(_variances(replace(prm, pbs_base_log=beta, pbs_level=lvl), group=grp)[0])
    act = R.active_steps(rows, N, n, grp)
    total = n if grp == 1 else (n + 1) // 2
    live = act > 0
    ratio = np.zeros(rows.shape[0])
    ratio[live] = np.abs(d[live]) / (sigma_model * np.sqrt(act[live] / total))
    print(f"one-hot {case}: max |delta| {np.abs(d).max() / sigma_model:.4f} sigma_model; in units of sigma_model * "
          f"sqrt(active / {total}): max {ratio.max():.3f}, rms {np.sqrt(np.mean(ratio[live] ** 2)):.3f} over "
          f"{int(live.sum())} rows; one active step: max {ratio[act == 1].max(initial=0):.3f} over "
          f"{int((act == 1).sum())}, two: max {ratio[act == 2].max(initial=0):.3f} over {int((act == 2).sum())}")
    assert np.array_equal(dec, (ph_ref + half) >> sh)
    assert np.array_equal(dec, (want + half) >> sh)
    assert np.abs(d).max() < 8 * sigma_model
    assert (~live).sum() > 0
    assert np.array_equal(out[~live], out_ref[~live])


# ------------------------------------------ e. noise-free sign extraction --
def sign_fixture(prm, oracle_lib, seed=1234):
    eng = Engine(prm, 0)
    eng.keygen(seed)
    return eng, R.keyless_oracle(oracle_lib, prm.as_dict())


def check_sign_ops(eng, ref, oracle_lib, big, P):
    """sign, bit_extract and threshold of trivial big rows: every output word
    (and the consumed ct_v) equals the oracle's."""
    v = (big[:, -1] + np.uint64(1 << (63 - P))).view(np.int64) >> (64 - P)
    top = np.where(v < 0, np.uint64(1 << 63), np.uint64(0))
    ct = eng.to_dev(big)
    sign = u64(eng.sign(ct))
    s_ref, cv_ref = R.oracle_sign_consuming(oracle_lib, ref, big)
    assert np.array_equal(sign, s_ref)
    assert np.array_equal(u64(ct), cv_ref)
    assert not sign[:, :-1].any() and np.array_equal(sign[:, -1], top)
    ct = eng.to_dev(big)
    refreshed, bsign = eng.bit_extract(ct)
    r_ref, b_ref, cv_ref = R.oracle_bit_extract_consuming(oracle_lib, ref, big)
    assert np.array_equal(u64(refreshed), r_ref)
    assert np.array_equal(u64(bsign), b_ref)
    assert np.array_equal(u64(ct), cv_ref)
    assert np.array_equal(b_ref[:, -1], top) and not b_ref[:, :-1].any()
    h = 1 << (P - 1)
    for T in (-h + 1, 0, h - 1):
        ok = (v - T >= -h) & (v - T < h)             # acc - T must fit msg_bits bits
        sub = np.ascontiguousarray(big[ok])
        ct = eng.to_dev(sub)
        bit = u64(eng.threshold(ct, T))
        assert np.array_equal(bit, ref.threshold(sub, T))
        assert np.array_equal(u64(ct), sub)          # fhe_threshold_batch keeps its input
        assert not bit[:, :-1].any()
        assert np.array_equal(bit[:, -1], np.where(v[ok] >= T, np.uint64(1 << 63), np.uint64(0)))


@pytest.mark.parametrize("P,dbits", [(8, 3), (8, 4), (7, 4), (5, 4), (4, 4)])
def test_sign_trivial_toy(need_gpu, oracle_lib, P, dbits):
    prm = replace(TOY, msg_bits=P, sign_digit_bits=dbits)
    eng, ref = sign_fixture(prm, oracle_lib)
    check_sign_ops(eng, ref, oracle_lib, R.trivial_big(prm.N, prm.k, P), P)
    eng.close()


@pytest.fixture(scope="module")
def sign_sets(need_gpu, oracle_lib):
    """params_for_bits(P) engines with keys and keyless oracles, made on demand."""
    made = {}

    def get(P):
        if P not in made:
            made[P] = sign_fixture(params_for_bits(P), oracle_lib) + (params_for_bits(P),)
        return made[P]
    yield get
    for eng, _, _ in made.values():
        eng.close()


@pytest.mark.parametrize("P", [16, 19, 26])
def test_sign_trivial_real(sign_sets, oracle_lib, P):
    """params_for_bits(16 / 19 / 26): every gadget family of the ladder (mid0,
    mid, mid2, fast, fast2) in the sign plan, the classic main gadget in the bit
    extraction. About 700 values and their two shifts: more than 2048 rows,
    past the two-stream split."""
    eng, ref, prm = sign_sets(P)
    big = R.trivial_big(prm.N, prm.k, P, max_rows=SIGN_ROWS)
    assert big.shape[0] >= 2048
    check_sign_ops(eng, ref, oracle_lib, big, P)


@pytest.mark.parametrize("count", [2047, 2048, 2051])
def test_sign_trivial_split_edges(sign_sets, oracle_lib, count):
    """Either side of PIPE_MIN = 2048, where sign_extract_batch goes from one
    stream to two halves, with a deterministic expectation."""
    eng, ref, prm = sign_sets(16)
    big = np.ascontiguousarray(R.trivial_big(prm.N, prm.k, 16, max_rows=SIGN_ROWS)[:count])
    ct = eng.to_dev(big)
    sign = u64(eng.sign(ct))
    s_ref, cv_ref = R.oracle_sign_consuming(oracle_lib, ref, big)
    assert np.array_equal(sign, s_ref)
    assert np.array_equal(u64(ct), cv_ref)


def test_sign_trivial_group(need_gpu, oracle_lib):
    """EngineGroup.sign with two tenants of unequal counts: the _grp rotation
    kernels and the grouped key switch, word for word."""
    engs = []
    for seed in (31, 32):
        e = Engine(REAL16, 0)
        e.keygen(seed)
        engs.append(e)
    ref = R.keyless_oracle(oracle_lib, REAL16.as_dict())
    grp = EngineGroup(engs)
    counts = [5, 130]
    M, starts = group_rows(counts)
    big = R.trivial_big(REAL16.N, REAL16.k, 16, max_rows=SIGN_ROWS)
    pick = (np.arange(sum(counts)) * 23 + 1) % big.shape[0]
    rows = np.zeros((M, engs[0].W), np.uint64)
    src = np.split(big[pick], [counts[0]])
    for s, c, part in zip(starts, counts, src):
        rows[s:s + c] = part
    ct = engs[0].to_dev(rows)
    sign = u64(grp.sign(ct, counts))
    assert engs[0].kernel_name("blind_rotate_fast") == "k_blind_rotate_mb_grp<2, 15>"
    assert engs[0].kernel_name("blind_rotate_fast2") == "k_blind_rotate_mb_grp<1, 23>"
    for s, c, part in zip(starts, counts, src):
        s_ref, cv_ref = R.oracle_sign_consuming(oracle_lib, ref, part)
        assert np.array_equal(sign[s:s + c], s_ref)
        assert not s_ref[:, :-1].any()
        assert np.array_equal(u64(ct)[s:s + c], cv_ref)
    grp.close()
    for e in engs:
        e.close()
