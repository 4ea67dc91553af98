"""Noise-free and near-noise-free inputs of the blind rotation, with their
closed forms (plain numpy and Python integers; no GPU).

A small LWE whose mask is zero meets no key: every step's exponent is 0, the
classic rotation decomposes X^0 ACC - ACC = 0 and the multi-bit one multiplies
by psi^0 - 1 = 0, so the bootstrap's output is the test vector rotated by the
switched body, sample-extracted: a zero mask and the body TV[switch(body)]
(negacyclic), exactly, in the oracle and on the GPU. `trivial_small` sweeps
every exponent and the rounding ties of the modulus switch; `trivial_expected`
restates the three test-vector kinds from include/fhe_icp.h (fhe_pbs_batch,
fhe_pbs_lut_batch, fhe_pbs_table_batch).

A mask with one or two nonzero words runs one or two external products: not
noise-free, but the oracle does it in milliseconds, and the words are chosen
(`onehot_small`) instead of drawn, so the exponent logic is tested at
a in {1, N - 1, N, N + 1, 2N - 1}, at the wrap 2N -> 0, at the first and last
mask index, and for the multi-bit rotation at every value of
e = switch(w1 + w2) - switch(w1) - switch(w2).
"""
import ctypes as C

import numpy as np

M64 = (1 << 64) - 1

# single words of the one-hot cases, in units of U = 2^64 / 2N (u) and of one
# torus word (c): w = u * U + c mod 2^64
#   U, (N-1)U, NU, (N+1)U, (2N-1)U, 2^64 - U/2 (rounds up to 2N: exponent 0),
#   U/2 - 1 (rounds down to 0), U/2 (the tie: rounds up to 1)
SINGLE_INDICES = 6    # {0, 1, 2, n - 3, n - 2, n - 1}
SINGLE_WORDS = 8
PAIR_WORDS = 8
PAIR_CHOICES = 6      # pair 0, the last full pair, the first pair of each key pattern
ONEHOT_CASES = SINGLE_INDICES * SINGLE_WORDS + PAIR_CHOICES * PAIR_WORDS    # 96, each at two bodies


def unit(N: int) -> int:
    """U = 2^64 / 2N: one step of the rotation exponent on the torus."""
    return (1 << 64) // (2 * N)


def switch(x, N: int) -> np.ndarray:
    """round(x * 2N / 2^64) mod 2N with ties up (the modulus switch), on
    uint64 words: x = q U + r, exponent q + [r >= U/2]."""
    x = np.asarray(x, dtype=np.uint64)
    U = np.uint64(unit(N))
    q, r = x // U, x % U
    return ((q + (r >= U // np.uint64(2)).astype(np.uint64)) % np.uint64(2 * N)).astype(np.int64)


def trivial_small(N: int, n: int) -> np.ndarray:
    """3 * 2N small LWEs (n + 1 words) with a zero mask: row 3 j + o has the
    body j U + off_o, off = (0, U/2 - 1, U/2): exactly on exponent j, the last
    word that still rounds down to j, and the tie, which rounds up to j + 1
    (to 0 at j = 2N - 1)."""
    U = unit(N)
    offs = (0, U // 2 - 1, U // 2)
    rows = np.zeros((3 * 2 * N, n + 1), np.uint64)
    body = [(j * U + off) & M64 for j in range(2 * N) for off in offs]
    rows[:, n] = np.array(body, dtype=np.uint64)
    return rows


def trivial_exponents(N: int) -> np.ndarray:
    """The exponents trivial_small's bodies switch to, stated directly."""
    return np.array([(j + o) % (2 * N) for j in range(2 * N) for o in (0, 0, 1)], dtype=np.int64)


def tv_at(kind, idx, N: int) -> np.ndarray:
    """Test vector coefficient idx in [0, 2N) of the negacyclic extension
    (TV[idx] for idx < N, -TV[idx - N] beyond), as uint64 words.

    kind is one of
      ("const", tv)                      fhe_pbs_batch: TV_j = tv
      ("stairs", base, step, log_slots)  fhe_pbs_lut_batch: 2^log_slots slots of
                                         N / 2^log_slots coefficients, slot s
                                         holding base + s * step
      ("table", lut, lut_bits, msg_bits) fhe_pbs_table_batch: box m is the
                                         N / 2^lut_bits coefficients within half a
                                         box of m * N / 2^lut_bits, holding
                                         lut[m] * 2^(64 - msg_bits); the half box
                                         left at the top is the image of the one
                                         below 0: -lut[0] * 2^(64 - msg_bits)
    """
    idx = np.asarray(idx, dtype=np.int64)
    j = idx % N
    if kind[0] == "const":
        v = [int(kind[1]) & M64 for _ in j.reshape(-1)]
    elif kind[0] == "stairs":
        _, base, step, log_slots = kind
        per = N >> log_slots
        v = [(int(base) + (int(x) // per) * int(step)) & M64 for x in j.reshape(-1)]
    elif kind[0] == "table":
        _, lut, lut_bits, msg_bits = kind
        box = N >> lut_bits
        delta = 1 << (64 - msg_bits)
        v = []
        for x in j.reshape(-1):
            m = (int(x) + box // 2) // box
            v.append((int(lut[m]) * delta) & M64 if m < (1 << lut_bits) else (-int(lut[0]) * delta) & M64)
    else:
        raise ValueError(kind[0])
    v = np.array(v, dtype=np.uint64).reshape(idx.shape)
    return np.where(idx % (2 * N) < N, v, np.uint64(0) - v)


def trivial_expected(small, N: int, k: int, kind) -> np.ndarray:
    """The bootstrap of zero-mask small LWEs: big LWEs (k N + 1 words) with a
    zero mask and the body TV[switch(body)]."""
    small = np.asarray(small, dtype=np.uint64)
    assert not small[:, :-1].any(), "trivial_expected takes zero masks"
    out = np.zeros((small.shape[0], k * N + 1), np.uint64)
    out[:, -1] = tv_at(kind, switch(small[:, -1], N), N)
    return out


def _first_pair(s_small, pattern) -> int:
    s = np.asarray(s_small).astype(np.int64)
    for j in range(len(s) // 2):
        if (int(s[2 * j]), int(s[2 * j + 1])) == pattern:
            return j
    raise ValueError(f"the small key has no pair with the bits {pattern}")


def exact_exponent(small, s_small, N: int, group: int) -> np.ndarray:
    """The rotation's total exponent in the clear: switch(body) minus the
    switched mask words of the set key bits; the multi-bit rotation (group 2)
    switches the exact sum w1 + w2 of a pair whose key bits are both set (one
    rounding, not two)."""
    small = np.asarray(small, dtype=np.uint64)
    s = np.asarray(s_small).astype(np.int64)
    n = s.size
    a = switch(small[:, :n], N)
    tot = switch(small[:, n], N).copy()
    if group == 2:
        for j in range(n // 2):
            s1, s2 = int(s[2 * j]), int(s[2 * j + 1])
            if s1 and s2:
                with np.errstate(over="ignore"):
                    tot -= switch(small[:, 2 * j] + small[:, 2 * j + 1], N)
            elif s1:
                tot -= a[:, 2 * j]
            elif s2:
                tot -= a[:, 2 * j + 1]
        if n % 2:
            tot -= a[:, n - 1] * int(s[n - 1])
    else:
        tot -= a @ s
    return tot % (2 * N)


def pair_e(w1, w2, N: int) -> int:
    """e = switch(w1 + w2) - switch(w1) - switch(w2) mod 2N, as a signed value."""
    a1, a2 = int(switch(np.uint64(w1), N)), int(switch(np.uint64(w2), N))
    a12 = int(switch(np.uint64((int(w1) + int(w2)) & M64), N))
    e = (a12 - a1 - a2) % (2 * N)
    return e - 2 * N if e >= N else e


def onehot_small(N: int, n: int, s_small, body=None, group: int = 1):
    """The one- and two-hot case list: (rows uint64 [2 * ONEHOT_CASES, n + 1],
    cases), cases[i] = (mask indices, words) of rows 2 i and 2 i + 1.

    Single words, at the mask indices {0, 1, 2, n-3, n-2, n-1}:
      U, (N-1)U, NU, (N+1)U, (2N-1)U, 2^64 - U/2, U/2 - 1, U/2.
    Two words, at the pairs (2j, 2j+1) for j in {0, the last full pair, the
    first pair of s_small with the key bits (0,0), (0,1), (1,0), (1,1)}:
      (NU, NU), ((2N-1)U, (2N-1)U), (U, (2N-1)U), 5U + U/2 - 1 twice (e = +1),
      5U + U/2 twice (e = -1), U/2 - 1 twice (a1 = a2 = 0, a12 = 1),
      2^64 - U/2 twice (a1 = a2 = 0, a12 = 2N - 1), (U/2, 2^64 - U/2).

    Each case comes at two bodies whose exponents differ by 1: `body` and
    body + U; with body = None, the bodies that put the exact total exponent
    (exact_exponent, for the rotation of `group`) on N - 1 and N, the two
    sides of a constant test vector's sign flip.
    """
    U = unit(N)
    s = np.asarray(s_small).astype(np.int64)
    singles = [U, (N - 1) * U, N * U, (N + 1) * U, (2 * N - 1) * U, (1 << 64) - U // 2, U // 2 - 1, U // 2]
    pairs = [(N * U, N * U), ((2 * N - 1) * U, (2 * N - 1) * U), (U, (2 * N - 1) * U),
             (5 * U + U // 2 - 1, 5 * U + U // 2 - 1), (5 * U + U // 2, 5 * U + U // 2),
             (U // 2 - 1, U // 2 - 1), ((1 << 64) - U // 2, (1 << 64) - U // 2), (U // 2, (1 << 64) - U // 2)]
    assert len(singles) == SINGLE_WORDS and len(pairs) == PAIR_WORDS
    cases = [((i,), (w,)) for i in (0, 1, 2, n - 3, n - 2, n - 1) for w in singles]
    which = [0, n // 2 - 1] + [_first_pair(s, pat) for pat in ((0, 0), (0, 1), (1, 0), (1, 1))]
    cases += [((2 * j, 2 * j + 1), ws) for j in which for ws in pairs]
    assert len(cases) == ONEHOT_CASES
    rows = np.zeros((2 * len(cases), n + 1), np.uint64)
    for c, (idx, ws) in enumerate(cases):
        for i, w in zip(idx, ws):
            rows[2 * c:2 * c + 2, i] = np.uint64(w & M64)
    if body is not None:
        rows[0::2, n] = np.uint64(int(body) & M64)
        rows[1::2, n] = np.uint64((int(body) + U) & M64)
    else:
        used = exact_exponent(rows, s, N, group)      # minus the mask's share (the bodies are still 0)
        for r in range(rows.shape[0]):
            want = N - 1 + (r & 1)
            rows[r, n] = np.uint64(((want - int(used[r])) % (2 * N)) * U)
    return rows, cases


def active_steps(small, N: int, n: int, group: int) -> np.ndarray:
    """How many rotation steps of each row do any work: nonzero exponents
    (classic), or pairs with any of a1, a2, a12 nonzero (multi-bit)."""
    small = np.asarray(small, dtype=np.uint64)
    a = switch(small[:, :n], N)
    if group != 2:
        return (a != 0).sum(axis=1)
    m = n // 2
    with np.errstate(over="ignore"):
        a12 = switch(small[:, 0:2 * m:2] + small[:, 1:2 * m:2], N)
    act = ((a[:, 0:2 * m:2] != 0) | (a[:, 1:2 * m:2] != 0) | (a12 != 0)).sum(axis=1)
    if n % 2:
        act = act + (a[:, n - 1] != 0)
    return act


def trivial_big(N: int, k: int, P: int, max_rows: int = 4096) -> np.ndarray:
    """Trivial big LWEs (zero mask) with the bodies v 2^(64-P): every P-bit v
    for P <= 12, else a stride that gives at most max_rows values, always with
    -2^(P-1), -1, 0 and 2^(P-1) - 1; then the same set shifted by +2^(62-P) and
    by -2^(62-P) (a quarter of a message step either way)."""
    h = 1 << (P - 1)
    if P <= 12:
        vs = list(range(-h, h))
    else:
        stride = -(-(2 * h) // (max_rows - 4))
        vs = sorted(set(range(-h, h, stride)) | {-h, -1, 0, h - 1})
        assert len(vs) <= max_rows
    q = 1 << (62 - P)
    body = [((v << (64 - P)) + d) & M64 for d in (0, q, -q) for v in vs]
    out = np.zeros((len(body), k * N + 1), np.uint64)
    out[:, -1] = np.array(body, dtype=np.uint64)
    return out


def keyless_oracle(oracle_lib, params: dict):
    """A RefTFHE of these parameters without key generation: every key is
    zero words (untouched pages). Only for inputs that never meet a key, the
    zero masks of this module; tests/test_rotation_exact_cpu.py checks on real
    keys that the oracle's result for them does not depend on the key."""
    L = oracle_lib.lib()
    ref = object.__new__(oracle_lib.RefTFHE)
    ref.params = {f: int(params.get(f, 0) if f in oracle_lib.OPTIONAL else params[f]) for f in oracle_lib.FIELDS}
    ref.P = oracle_lib.RefParams(**ref.params)
    ref.n, ref.k, ref.N = ref.params["n"], ref.params["k"], ref.params["N"]
    ref.big = ref.k * ref.N
    ref.s_small = np.zeros(ref.n, np.uint64)
    ref.s_big = np.zeros(ref.big, np.uint64)
    ref.bsk = np.zeros(L.ref_bsk_words(C.byref(ref.P)), np.uint64)
    ref.ksk = np.zeros(L.ref_ksk_words(C.byref(ref.P)), np.uint64)
    ref.keys = {g: np.zeros(L.ref_bsk2_words(C.byref(ref.P), g), np.uint64)
                for g, lv in oracle_lib.GADGET_LEVEL.items() if ref.params[lv]}
    ref.bsk2, ref.bsk3 = ref.keys.get(1), ref.keys.get(2)
    return ref


def _keys5(ref, u64p):
    return (u64p * 5)(*[ref.keys[g].ctypes.data_as(u64p) if g in ref.keys else None for g in range(1, 6)])


def oracle_sign_consuming(oracle_lib, ref, ct_v):
    """ref.sign_extract, but also returning the consumed ct_v:
    (sign, ct_v after the call)."""
    u64p = C.POINTER(C.c_uint64)
    cv = np.array(ct_v, dtype=np.uint64, copy=True, order="C")
    cnt = cv.size // (ref.big + 1)
    sign = np.zeros((cnt, ref.big + 1), np.uint64)
    oracle_lib.lib().ref_sign_extract_keys(C.byref(ref.P), oracle_lib.u64(ref.bsk), _keys5(ref, u64p),
                                           oracle_lib.u64(ref.ksk), oracle_lib.u64(cv), cnt, oracle_lib.u64(sign))
    return sign, cv.reshape(cnt, ref.big + 1)


def oracle_bit_extract_consuming(oracle_lib, ref, ct_v):
    """ref.bit_extract, but also returning the consumed ct_v:
    (refreshed, sign, ct_v after the call)."""
    cv = np.array(ct_v, dtype=np.uint64, copy=True, order="C")
    cnt = cv.size // (ref.big + 1)
    refreshed = np.zeros((cnt, ref.big + 1), np.uint64)
    sign = np.zeros((cnt, ref.big + 1), np.uint64)
    oracle_lib.lib().ref_bit_extract(C.byref(ref.P), oracle_lib.u64(ref.bsk), oracle_lib.u64(ref.ksk),
                                     oracle_lib.u64(cv), cnt, oracle_lib.u64(refreshed), oracle_lib.u64(sign))
    return refreshed, sign, cv.reshape(cnt, ref.big + 1)
