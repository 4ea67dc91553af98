"""GPU: rotation schedules in the stored-ciphertext hub.

fhe_bridge_group_gens_batch on the padded rows of a group is, segment by
segment, word for word the numpy restatement (tests/bridge_ref.py) with each
(tenant, generation)'s key, and each tenant's segment is what
fhe_bridge_gens_batch gives on its own context: with and without the GEMM's K
split, on the bridge's edge words at segment boundaries, on degenerate maps, on
two gadget classes in one call, and once at the P = 16 parameters. Canaries on
every current-key row, every padding row and one row past the buffer survive.
The entries' refusals in their order (the FHE_E_ARG order is checked here and
not on the CPU: a group needs contexts with evaluation keys). And
CorpusHub(rotation_schedules=True) end to end on the toy model.

All arithmetic is modulo 2^64: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import bridge_ref as BR
from oracle import quant_ref as Q

from fheicp import _lib
from fheicp.engine import Engine, EngineGroup, group_rows
from fheicp.params import TOY, bridge_plan, params_for_bits
from test_gpu_bridge_gens import CANARY, EDGE_WORDS, dev_u64, host_u64, s_big_of, segment_rows, toy_model

pytestmark = pytest.mark.gpu

U = np.uint64
BETA, LV = 4, 3
# generation g of tenant t -> bridge slot: a different permutation per tenant, none the identity
PERMS = ([3, 7, 0, 5, 1, 6, 2, 4], [1, 0, 3, 2, 5, 4, 7, 6], [7, 6, 5, 4, 3, 2, 1, 0])


class Tenants:
    """Engines with their own evaluation keys in one group; keys[t][slot] is
    the numpy-made bridge key (uniform words) in that slot, gadget[t][slot]
    its (base_log, level)."""

    def __init__(self, params, seeds):
        self.engines = []
        for s in seeds:
            e = Engine(params, 0)
            e.keygen(s)
            self.engines.append(e)
        self.keys = [{} for _ in seeds]
        self.gadget = [{} for _ in seeds]
        self.group = EngineGroup(self.engines)
        self.W = self.engines[0].W

    def put(self, t, slot, key, beta=BETA, lv=LV):
        self.engines[t].import_bridge_key(beta, lv, key, slot=slot)
        self.keys[t][slot], self.gadget[t][slot] = key, (beta, lv)

    def close(self):
        self.group.close()
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def toy3(need_gpu):
    """Three TOY tenants, each with eight distinct keys of uniform words,
    gadget (4, 3): tenant t's generation g sits in slot PERMS[t][g]."""
    ten = Tenants(TOY, (301, 302, 303))
    rng = np.random.default_rng(2025)
    big = TOY.k * TOY.N
    for t in range(3):
        for g in range(8):
            ten.put(t, PERMS[t][g], rng.integers(0, 2 ** 64, (big, LV, big + 1), dtype=U))
        assert ten.engines[t].bridge_slots() == list(range(8))
    yield ten
    ten.close()


def layout(maps):
    """(M, starts, per tenant the padded-buffer rows of each segment)."""
    M, starts = group_rows([0 if m is None else m[0] * m[1] for m in maps])
    segs = [None if m is None else [idx + starts[t] for idx in segment_rows(m[0], m[1], m[2])]
            for t, m in enumerate(maps)]
    return M, starts, segs


def canaried(rng, ten, maps):
    """Random words on every old generation's rows, the canary word on every
    current-key row, every padding row and the row after the buffer."""
    M, _, segs = layout(maps)
    ct = np.full((M + 1, ten.W), CANARY, dtype=U)
    for s in segs:
        for idx in s or ():
            if idx.size:
                ct[idx] = rng.integers(0, 2 ** 64, (idx.size, ten.W), dtype=U)
    return ct


def check_group(ten, maps, ct, brackets=1, expect_rows=None):
    """maps: per tenant None or (Q, B, ends, slots); ct [M + 1, W] with a
    canary last. Runs the group entry in place and compares the whole buffer
    with the restatement, and every tenant's segment with its own context."""
    M, starts, segs = layout(maps)
    want = np.array(ct, copy=True)
    for t, m in enumerate(maps):
        for g, idx in enumerate(segs[t] or ()):
            if idx.size:
                slot = m[3][g]
                want[idx] = BR.bridge_ref(ct[idx], ten.keys[t][slot], *ten.gadget[t][slot])
    x = dev_u64(ten.engines[0], ct)
    e0 = ten.engines[0]
    e0.profile(True)
    try:
        ten.group.bridge_gens(x, maps)
        prof = e0.profile_read("bridge")
    finally:
        e0.profile(False)
    bridged = [idx for s in segs for idx in (s or ()) if idx.size]
    bridged = np.concatenate(bridged) if bridged else np.zeros(0, np.int64)
    rows = len(bridged)
    if expect_rows is not None:
        assert rows == expect_rows
    # one bracket per pass in the first context's bucket, items = the rows bridged
    assert (prof["launches"], prof["items"]) == ((brackets, rows) if rows else (0, 0))
    got = host_u64(x)
    np.testing.assert_array_equal(got, want)
    assert rows == 0 or not np.array_equal(got[bridged], ct[bridged])
    untouched = np.setdiff1d(np.arange(M + 1), bridged)
    assert (got[untouched] == U(CANARY)).all()
    # each tenant's segment against fhe_bridge_gens_batch on its own context
    for t, m in enumerate(maps):
        if m is None:
            continue
        n = m[0] * m[1]
        own = dev_u64(ten.engines[t], ct[starts[t]:starts[t] + n])
        ten.engines[t].bridge_gens(own, *m)
        np.testing.assert_array_equal(got[starts[t]:starts[t] + n], host_u64(own), err_msg=f"tenant {t}")
    return got


def slots_of(t, G):
    return PERMS[t][:G]


SPLIT = [(1, 301, [129, 150, 290], slots_of(0, 3)), None, (3, 7, [2, 2, 5], slots_of(2, 3))]
UNSPLIT = [(2, 301, [129, 150, 290], slots_of(0, 3)), None, (3, 7, [2, 2, 5], slots_of(2, 3))]


def blocks_of(maps):
    return sum(-(-m[0] * (e - (m[2][g - 1] if g else 0)) // 128)
               for m in maps if m is not None for g, e in enumerate(m[2]))


def test_group_bridge_split_path_bit_exact_toy(toy3):
    """Tenant 0: 129 | 21 | 140 rows (every segment ends in a partial block, a
    16-row digit group is crossed), 11 current-key documents, 3 padding rows
    before tenant 2; tenant 1 sits out; tenant 2: 6 | 0 | 9 rows. 5 + 2 = 7
    blocks x 33 column blocks = 231 tiles <= 256: the GEMM splits K and adds
    atomically into compact rows the digits kernel zeroed."""
    assert blocks_of(SPLIT) == 7 and 7 * 33 <= 256
    M, starts, _ = layout(SPLIT)
    assert starts == [0, 304, 304] and M == 304 + 24
    rng = np.random.default_rng(11)
    check_group(toy3, SPLIT, canaried(rng, toy3, SPLIT), expect_rows=290 + 15)
    assert toy3.engines[0].kernel_name("bridge") == "k_keyswitch_mfma_grp<8, 1>"


def test_group_bridge_unsplit_path_bit_exact_toy(toy3):
    """The same with tenant 0 at Q = 2: 258 | 42 | 280 rows are 3 + 1 + 3
    blocks, with tenant 2's two 9 blocks, 297 tiles > 256: the split rule
    leaves S = 1 and the GEMM stores instead of adding."""
    assert blocks_of(UNSPLIT) == 9 and 9 * 33 > 256 >= 7 * 33
    rng = np.random.default_rng(12)
    check_group(toy3, UNSPLIT, canaried(rng, toy3, UNSPLIT), expect_rows=580 + 15)


def test_group_bridge_edge_words_at_segment_boundaries(toy3):
    """The edge words (digits at both ends of their range, ties with both
    coins) on the first and last document of every segment of both tenants."""
    rng = np.random.default_rng(13)
    ct = canaried(rng, toy3, SPLIT)
    _, starts, _ = layout(SPLIT)
    for i, b in enumerate((0, 128, 129, 149, 150, 289)):
        ct[starts[0] + b, :] = U(EDGE_WORDS[i % 4])
    for q in range(3):
        for i, b in enumerate((0, 1, 2, 4)):
            ct[starts[2] + q * 7 + b, :] = U(EDGE_WORDS[(i + q) % 4])
    check_group(toy3, SPLIT, ct)


def test_group_bridge_degenerate_maps_in_one_call(toy3):
    """Eight generations of one row each; a tenant at G = 0; a tenant at
    G = 1, slot 0, whose segment is fhe_bridge_rows_batch's words."""
    maps = [(1, 9, [1, 2, 3, 4, 5, 6, 7, 8], slots_of(0, 8)), (2, 3, [], []), (3, 7, [2], [0])]
    rng = np.random.default_rng(14)
    ct = canaried(rng, toy3, maps)
    got = check_group(toy3, maps, ct, expect_rows=8 + 6)
    _, starts, _ = layout(maps)
    own = dev_u64(toy3.engines[2], ct[starts[2]:starts[2] + 21])
    toy3.engines[2].bridge_rows(own, 3, 7, 2)
    np.testing.assert_array_equal(got[starts[2]:starts[2] + 21], host_u64(own))
    # every tenant sitting out, or at G = 0: nothing to do, nothing recorded
    for maps in ([None, None, None], [(2, 3, [], []), None, (1, 4, [0], [5])]):
        check_group(toy3, maps, canaried(rng, toy3, maps), expect_rows=0)


@pytest.fixture(scope="module")
def two_gadgets(need_gpu):
    """Tenant 0's keys at (4, 3) in slots 0 and 1, tenant 1's at (7, 6) in
    slots 0 and 1; slot 5 is empty on both."""
    ten = Tenants(TOY, (401, 402))
    rng = np.random.default_rng(2026)
    big = TOY.k * TOY.N
    for t, (beta, lv) in enumerate(((4, 3), (7, 6))):
        for slot in (0, 1):
            ten.put(t, slot, rng.integers(0, 2 ** 64, (big, lv, big + 1), dtype=U), beta, lv)
    yield ten
    ten.close()


def test_group_bridge_two_gadget_classes(two_gadgets):
    """One pass per distinct gadget, in order of first appearance: two
    brackets; every segment equals the restatement at its own gadget and its
    own context's result."""
    maps = [(2, 20, [17, 19], [1, 0]), (1, 130, [129, 130], [0, 1])]
    rng = np.random.default_rng(15)
    check_group(two_gadgets, maps, canaried(rng, two_gadgets, maps), brackets=2, expect_rows=38 + 130)


def test_group_bridge_state_refusals_write_nothing(two_gadgets):
    ten = two_gadgets
    rng = np.random.default_rng(16)
    maps = [(2, 4, [1, 3], [0, 1]), (1, 6, [2, 5], [1, 5])]
    ct = rng.integers(0, 2 ** 64, (layout(maps)[0] + 1, ten.W), dtype=U)
    x = dev_u64(ten.engines[0], ct)
    with pytest.raises(_lib.FheError, match="FHE_E_STATE.*tenant 1: no bridge key in slot 5"):
        ten.group.bridge_gens(x, maps)
    ten.group.bridge_gens(x.clone(), [maps[0], (1, 6, [2, 2], [1, 5])])        # ... unless the slot has no rows
    # differing gadgets inside one tenant
    big = TOY.k * TOY.N
    ten.put(0, 2, rng.integers(0, 2 ** 64, (big, 6, big + 1), dtype=U), 7, 6)
    try:
        with pytest.raises(_lib.FheError, match="FHE_E_STATE.*tenant 0: bridge gadgets differ"):
            ten.group.bridge_gens(x, [(2, 4, [1, 3], [0, 2]), (1, 6, [2, 5], [1, 0])])
    finally:
        ten.engines[0].drop_bridge_key(2)
        del ten.keys[0][2], ten.gadget[0][2]
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u64(x), ct)                             # nothing was written


def test_group_entries_argument_order(toy3):
    """FHE_E_ARG first, naming the tenant, before any key is looked at; then
    FHE_E_STATE; then the launch limit. Tenants at Q = 0 are skipped whatever
    else their records hold."""
    L, grp = toy3.group._L, toy3.group
    x = torch.zeros(4096, dtype=torch.int64, device=toy3.engines[0].device)
    p = x.data_ptr()
    err = lambda: L.fhe_last_error(None)  # noqa: E731
    ok = C.sizeof(_lib.FheGroupRowmap)
    e24, e99, s01, s00, s09 = ((C.c_int64 * 2)(2, 4), (C.c_int64 * 2)(3, 2), (C.c_int32 * 2)(0, 1),
                               (C.c_int32 * 2)(3, 3), (C.c_int32 * 2)(0, 9))

    def maps(*recs):
        arr = (_lib.FheGroupRowmap * 3)()
        for t, (size, Qn, B, G, ends, slots) in enumerate(recs):
            a = arr[t]
            a.struct_size, a.Q, a.B, a.G = size, Qn, B, G
            a.h_ends = C.addressof(ends) if ends is not None else None
            a.h_slots = C.addressof(slots) if slots is not None else None
        return arr
    good = (ok, 1, 4, 2, e24, s01)
    out = (ok, 0, -5, 99, None, None)                                  # sits out: nothing else is read
    bridge = lambda m, ct=p, T=3: L.fhe_bridge_group_gens_batch(grp._grp, ct, m, T, None)  # noqa: E731
    assert bridge(maps(good, (ok - 8, 1, 4, 2, e24, s01), good)) == -1 and b"tenant 1" in err()
    assert b"struct_size" in err()
    assert bridge(maps(good, good, (ok, -1, 4, 0, None, None))) == -1 and b"tenant 2: Q < 0" in err()
    for Qn, B in ((1, 0), (2 ** 31, 4), (2 ** 16, 2 ** 16)):
        assert bridge(maps(out, (ok, Qn, B, 0, None, None), good)) == -1
        assert b"tenant 1" in err() and b"bridge generations" in err()
    for bad, why in (((ok, 1, 4, 9, e24, s01), b"G outside [0, 8]"), ((ok, 1, 4, -1, e24, s01), b"G outside [0, 8]"),
                     ((ok, 1, 4, 2, None, s01), b"null bridge generations tables"),
                     ((ok, 1, 4, 2, e24, None), b"null bridge generations tables"),
                     ((ok, 1, 4, 2, e99, s01), b"ends must not decrease"),
                     ((ok, 1, 3, 2, e24, s01), b"ends must not decrease"),
                     ((ok, 1, 4, 2, e24, s09), b"bridge slot 9"), ((ok, 1, 4, 2, e24, s00), b"slot 3 named twice")):
        assert bridge(maps(good, out, bad)) == -1 and b"tenant 2" in err() and why in err(), why
        # the row-map rules come before the null buffer
        assert bridge(maps(good, out, bad), ct=None) == -1 and b"null bridge buffers" in err() and b"tenant 0" in err()
        assert bridge(maps(out, out, bad), ct=None) == -1 and why in err()
    assert bridge(maps(out, good, out), ct=None) == -1 and b"tenant 1: null bridge buffers" in err()
    assert bridge(maps((ok, 1, 2 ** 30, 0, None, None), (ok, 1, 2 ** 30, 0, None, None), good)) == -1
    assert b"2^31" in err()
    assert bridge(maps(good, good, good), T=2) == -1 and b"one fhe_group_rowmap per tenant" in err()
    assert bridge(None) == -1
    assert bridge(maps(out, out, out), ct=None) == 0                   # every tenant sits out
    # an argument error of a later tenant comes before an earlier tenant's missing key
    toy3.engines[0].drop_bridge_key(0)
    try:
        assert bridge(maps(good, out, (ok, 1, 4, 9, e24, s01))) == -1 and b"tenant 2" in err()
        assert bridge(maps(good, out, good)) == -3 and b"tenant 0: no bridge key in slot 0" in err()
    finally:
        big = TOY.k * TOY.N
        toy3.put(0, 0, np.random.default_rng(5).integers(0, 2 ** 64, (big, LV, big + 1), dtype=U))
    # the launch limit over all segments of a pass, before anything is queued (the buffer is never touched):
    # 2 x ceil(600000 / 128) = 9376 blocks > 8191, each tenant alone below it
    e6 = (C.c_int64 * 1)(600000)
    s0 = (C.c_int32 * 1)(0)
    huge = (ok, 1, 600000, 1, e6, s0)
    assert bridge(maps(huge, out, huge)) == -1 and b"split the call" in err()
    # the search entry: its own bounds, levels_bit, the row map, nulls; then the packing key (these engines hold none)
    key = (C.c_uint32 * 8)()
    hT = (C.c_int64 * 2)(0, 0)
    okc = C.sizeof(_lib.FheGroupCorpusGens)

    def items(Qs=(1, 1, 1), sizes=(okc,) * 3, B=4, D=5, G=2, ends=e24, slots=s01):
        arr = (_lib.FheGroupCorpusGens * 3)()
        for t in range(3):
            a = arr[t]
            a.struct_size, a.D, a.Q, a.B, a.G = sizes[t], D, Qs[t], B, G
            a.d_body = a.d_id0 = a.d_W = a.d_glwe_acc = a.d_glwe_bit = p
            a.h_mask_key, a.h_T = C.addressof(key), C.addressof(hT)
            a.h_ends, a.h_slots = C.addressof(ends), C.addressof(slots)
        return arr
    search = lambda a, T=3: L.fhe_search_seeded_queries_group_gens_batch(grp._grp, a, T, None)  # noqa: E731
    assert search(items(sizes=(okc, okc - 8, okc))) == -1 and b"tenant 1" in err() and b"struct_size" in err()
    assert search(items(Qs=(0, -1, 0))) == -1 and b"tenant 1: Q < 0" in err()
    assert search(items(D=0)) == -1 and b"tenant 0" in err() and b"seeded queries" in err()
    a = items(G=9)
    a[2].levels_bit = 9
    a[2].h_T = None
    assert search(a) == -1 and b"tenant 0" in err() and b"G outside" in err()
    a[0].G = a[1].G = 2
    assert search(a) == -1 and b"tenant 2" in err() and b"levels_bit" in err()
    a[2].levels_bit = 0
    assert search(a) == -1 and b"tenant 2" in err() and b"G outside" in err()     # the row map before the nulls
    a[2].G = 2
    assert search(a) == -1 and b"tenant 2: null search arguments" in err()
    assert search(items(slots=s00)) == -1 and b"named twice" in err()
    a = items(B=2 ** 30, D=1, G=0)
    assert search(a) == -1 and b"2^31" in err()
    assert search(items(), T=2) == -1 and b"one fhe_group_corpus_gens per tenant" in err()
    assert search(items(Qs=(0, 1, 0))) == -3 and b"tenant 1" in err() and b"packing key" in err()
    assert search(items(Qs=(0, 0, 0), G=99)) == 0


# ----------------------------------------- real parameters, sampled columns --
def test_group_bridge_sampled_columns_p16(need_gpu):
    """Two tenants on the P = 16 parameters with the planned bridge gadget
    (test_bridge_gens_sampled_columns_p16's construction): tenant 0 holds a
    bridge from A's key in slot 0 and one from a third key in slot 1, (1, 300,
    [129, 300]); tenant 1 one from a fourth key, (1, 5, [5]). Sixty-four
    sampled columns plus the body against the restatement on the exported
    keys' columns, and A's messages decrypt under tenant 0's key."""
    p = params_for_bits(16)
    beta, lv = bridge_plan(p, 0.0)
    A = Engine(p, 0)
    A.keygen(501)
    ten = Tenants(p, (502, 503))
    T0, T1 = ten.engines
    big = p.k * p.N
    rng = np.random.default_rng(16)
    T0.keygen_bridge_key(s_big_of(A), beta, lv, seed=9)
    T0.keygen_bridge_key(rng.integers(0, 2, big, dtype=U), beta, lv, seed=10, slot=1)
    T1.keygen_bridge_key(rng.integers(0, 2, big, dtype=U), beta, lv, seed=11)
    maps = [(1, 300, [129, 300], [0, 1]), (1, 5, [5], [0])]
    M, starts, segs = layout(maps)
    assert starts == [0, 300] and M == 308
    P = p.msg_bits
    msgs = rng.integers(-(1 << (P - 1)), 1 << (P - 1), 129)
    ct = rng.integers(0, 2 ** 64, (M + 1, big + 1), dtype=U)
    ct[:129] = host_u64(A.encrypt(msgs, seed=12, id0=3)).reshape(129, big + 1)
    ct[200, :] = U(0x8080808080808080)
    ct[305:] = U(CANARY)                                               # tenant 1's padding rows and the row past M
    cols = np.unique(np.concatenate([rng.choice(np.arange(1, big - 1), 62, replace=False), [0, big - 1, big]]))
    assert len(cols) == 65 and cols[-1] == big       # 64 mask columns, both ends among them, and the body
    want = np.array(ct[:, cols], copy=True)
    for (t, slot), idx in zip(((0, 0), (0, 1), (1, 0)), segs[0] + segs[1]):
        bk = ten.engines[t].export_bridge_key(slot).reshape(big, lv, big + 1)
        want[idx] = BR.bridge_ref(ct[idx], bk, beta, lv, cols=cols)
        del bk
    x = dev_u64(T0, ct)
    ten.group.bridge_gens(x, maps)
    got = host_u64(x)
    np.testing.assert_array_equal(got[:, cols], want)
    assert (got[305:] == U(CANARY)).all()
    np.testing.assert_array_equal(T0.decrypt(x[:129]).cpu().numpy(), msgs)
    A.close()
    ten.close()


# ------------------------------------------------------------ end to end --
HUB_DOC_SEED, HUB_QUERIES = 3, np.array([[1, -2, 1, 1, -1], [1, 1, 1, 1, 1]], np.float32)
HUB_PARTS = {"alice": (12, 17, 20), "bob": (6, 10), "carol": (9,)}      # the generations' ends, the last one current


def hub_case():
    """Clear data of the end-to-end case, no device: per tenant (docs, ts,
    ref accumulators, expected bits). Thresholds at the medians."""
    cq, oq = toy_model()
    rng = np.random.default_rng(HUB_DOC_SEED)
    out = {}
    for name, ends in HUB_PARTS.items():
        docs = rng.integers(-2, 2, (ends[-1], 5)).astype(np.float32)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, cq.n_e, q, docs) for q in HUB_QUERIES])
        sc = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        ts = [float(np.median(sc[0])), float(np.median(sc[1])) + 0.5]
        below = np.stack([(sc[i] < t).astype(np.int64) for i, t in enumerate(ts)])
        out[name] = (docs, ts, ref, below)
    return cq, oq, out


def assert_bits_on_both_sides(case):
    for name, ends in HUB_PARTS.items():
        below = case[name][3]
        for lo, hi in zip((0,) + ends, ends):
            for q in range(len(HUB_QUERIES)):
                assert 0 < below[q, lo:hi].sum() < hi - lo, (name, q, lo, hi)


def test_hub_rotation_schedules_end_to_end_toy(need_gpu):
    """alice lived through two rotations (12 + 5 + 3 documents, direct bridges
    from both earlier clients), bob was rotated once and appended to (his keys
    travel in the seeded form), carol was never rotated."""
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusHub
    cq, oq, case = hub_case()
    assert_bits_on_both_sides(case)
    hub, plain = CorpusHub(0, rotation_schedules=True), CorpusHub(0)
    clients, old = {}, {}

    def first(name, i, seeded=False):
        c = EncryptedCorpus(cq, TOY).compile(key_seed=50 + i, device=0, noise_seed=60 + i,
                                             mask_key=np.arange(8, dtype=np.uint32) + 41 + i, seeded_keys=seeded,
                                             key_mask_seed=700 if seeded else None)
        client = CorpusClient(c, pack_seed=70 + i)
        for h in (hub,) if name == "alice" else (hub, plain):
            h.add_tenant(name, client.eval_keys(), cq, c.P0, c.mask_key, scheme=c.scheme)
        return client

    def each(name, f):
        for h in (hub,) if name == "alice" else (hub, plain):
            f(h)
    docs = case["alice"][0]
    a0 = first("alice", 0)
    hub.load("alice", *a0.encrypt_docs(docs[:12], id0=np.arange(12, dtype=U) * U(5) + U(1000)))
    a1 = a0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
    hub.rekey("alice", a1.eval_keys())
    hub.append("alice", *a1.encrypt_docs(docs[12:17]))
    a2 = a1.rotate(key_seed=9, pack_seed=21, bridge_seed=22, noise_seed=23, bridge_from=[a0, a1])
    hub.rekey("alice", a2.eval_keys())                                 # a multi-bridge dict: accepted
    hub.append("alice", *a2.encrypt_docs(docs[17:]))
    clients["alice"], old["alice"] = a2, a1
    assert hub.tenants["alice"].generations == [(a0.key_id, 12), (a1.key_id, 17), (a2.key_id, 20)]
    docs = case["bob"][0]
    b0 = first("bob", 1, seeded=True)
    enc = b0.encrypt_docs(docs[:6], id0=np.arange(6, dtype=U) * U(5) + U(5000))
    each("bob", lambda h: h.load("bob", *enc))
    b1 = b0.rotate(key_seed=84, pack_seed=85, bridge_seed=86, noise_seed=87)
    keys1 = b1.eval_keys()
    assert "bsk_body" in keys1 and "bridge_key_body" in keys1
    each("bob", lambda h: h.rekey("bob", keys1))
    enc = b1.encrypt_docs(docs[6:])
    each("bob", lambda h: h.append("bob", *enc))
    clients["bob"], old["bob"] = b1, b0
    c0 = first("carol", 2)
    enc = c0.encrypt_docs(case["carol"][0], id0=np.arange(9, dtype=U) * U(5) + U(9000))
    each("carol", lambda h: h.load("carol", *enc))
    clients["carol"] = c0
    assert [CorpusHub.gen_map(s) for s in hub.tenants.values()] == [([12, 17], [0, 1]), ([6], [0]), ([], [])]
    requests = {name: (HUB_QUERIES, case[name][1]) for name in HUB_PARTS}
    assert [r["mode"] for r in hub.rounds(requests)] == ["group"]
    e0 = hub.tenants["alice"].engine
    e0.profile(True)
    try:
        got = hub.search_many(requests)
        prof = e0.profile_read("bridge")
    finally:
        e0.profile(False)
    # alice's two old generations and bob's one in ONE grouped pass: 2 x (12 + 5 + 6) rows
    assert (prof["launches"], prof["items"]) == (1, 46) and e0.kernel_name("bridge") == "k_keyswitch_mfma_grp<8, 1>"
    for name in HUB_PARTS:
        docs, ts, ref, below = case[name]
        acc, bits = clients[name].decrypt_replies(got[name])
        np.testing.assert_array_equal(acc.cpu().numpy(), ref, err_msg=name)
        np.testing.assert_array_equal(bits.cpu().numpy(), below, err_msg=name)
        own = hub.tenants[name].search_many(HUB_QUERIES, ts)
        assert len(own) == len(got[name])
        for a, b in zip(got[name], own):
            pa, pb = int(a[1]) >> 32, int(b[1]) >> 32               # the replies' width fields
            assert pa >= pb
            if pa == pb:
                np.testing.assert_array_equal(a, b, err_msg=f"{name}: reply words against its own server")
    # a rotated-out client cannot open them
    for name, client in old.items():
        acc, _ = client.decrypt_replies(got[name])
        assert not np.array_equal(acc.cpu().numpy(), case[name][2]), name
    # every tenant at G <= 1: the replies are a default hub's word for word
    two = {n: requests[n] for n in ("bob", "carol")}
    assert [r["mode"] for r in hub.rounds(two)] == [r["mode"] for r in plain.rounds(two)] == ["group"]
    a, b = hub.search_many(two), plain.search_many(two)
    for n in two:
        assert len(a[n]) == len(b[n]) == 1
        np.testing.assert_array_equal(a[n][0], b[n][0], err_msg=f"{n}: against the default hub")
    acc, bits = clients["bob"].decrypt_replies(a["bob"])
    np.testing.assert_array_equal(acc.cpu().numpy(), case["bob"][2])
    hub.close()
    plain.close()
