"""GPU: libfheicp's encoder (fhe-icp_amd/csrc/bert.hip) against the float64
restatement tests/bert_ref.py (pinned to transformers by
tests/test_bert_ref_cpu.py) on the shapes of bert_ref.CASES, where its kernels
change path: 1 to 48 K steps of the GEMM pipelines, N % 128 == 64, M below one
tile, fewer blocks than XCDs, both attention kernels' later query blocks,
k_attention<4>, wholly masked key chunks, a mask with holes, S = 1 and
S = 512, both LayerNorm kernels at their widest rows. The weights have
non-zero biases, LayerNorm gains and shifts and give attention logits of std
2 to 3. Every comparison runs over all B * S positions, padded ones included
(max pooling reads them).

Bounds (test_hidden_state_vs_f64): the error of a CPU restatement in the
same arithmetic against float64 is the yardstick, on the same case and in the
same two metrics (relative RMS of the whole tensor; the worst relative RMS of
one token's row), and the GPU may be R (f32) or RB (bf16) times that.
R and RB are twice the largest ratio measured on an MI355X, rounded up to a
power of two, and must stay within what the arithmetic explains: R <= 16 (a
sequential f32 chain over K <= 3072 against torch's blocked sums), RB <= 2
(the same roundings; erf to 1.5e-7, __expf and v_rcp_f32 lie far below 2^-9).

Measured on an MI355X, GPU error / yardstick as (rel RMS, worst token)
(docs/AB_LOG_r10.md has the absolute figures):

  case     f32            bf16
  s1       1.42  1.27     1.00  1.00
  s65      1.02  1.00     1.00  0.99
  s129     1.31  1.24     1.00  1.02
  s257     1.14  0.86     0.99  0.97
  s512     1.10  0.94     1.00  0.96
  s200     1.02  0.96     0.99  0.99
  h1024    2.01  2.29     0.96  0.98
  h960     1.89  1.93     0.98  0.96
  base1    2.26  2.12     0.99  0.94

R = 8: twice the largest f32 ratio (2.29) is 4.58. RB = 2: the largest bf16
ratio is 1.02; the rule would give 4 (2.04 rounded up), which the condition
RB <= 2 does not admit, so RB stays at the condition's 2, a factor 1.96 above
anything measured. The f32 yardsticks are 1.5e-7 to 3.4e-7 (rel RMS) and
1.7e-7 to 7.1e-7 (worst token), the bf16 ones 2.5e-3 to 3.3e-3 and 2.9e-3 to
5.6e-3: an error of 1e-3 in f32, or a few percent in bf16, fails.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bert_ref as R

pytestmark = pytest.mark.gpu

R_F32, R_BF16 = 8.0, 2.0
PRECISIONS = ("f32", "bf16")
E_ARG, E_STATE = -1, -3


class _Case:
    """One case's weights, inputs, float64 reference and yardsticks (computed
    once on the CPU, never modified) and its GPU handles."""

    def __init__(self, name):
        self.name = name
        self.cfg, self.sd = R.case_weights(name)
        self.ids, self.mask, self.tt = R.make_inputs(name)
        self.ref = R.forward(self.sd, self.cfg, self.ids, self.mask, self.tt)
        like = {"f32": R.forward(self.sd, self.cfg, self.ids, self.mask, self.tt, dtype=torch.float32),
                "bf16": R.forward(self.sd, self.cfg, self.ids, self.mask, self.tt, rnd=R.bf16)}
        self.yard = {p: (R.rel_rms(x, self.ref), R.worst_token(x, self.ref)) for p, x in like.items()}
        self._gpu, self._hid = {}, {}

    def gpu(self, precision):
        if precision not in self._gpu:
            from fheicp.bert import GpuBert
            self._gpu[precision] = GpuBert(state_dict=self.sd, config=self.cfg, device=0, precision=precision)
        return self._gpu[precision]

    def hidden(self, precision):
        """the GPU's last_hidden_state of the case's inputs, on the host"""
        if precision not in self._hid:
            self._hid[precision] = self.gpu(precision).forward(self.ids, self.mask, self.tt, pooling="none").cpu()
        return self._hid[precision]

    def bound(self, precision):
        f = R_F32 if precision == "f32" else R_BF16
        return f * self.yard[precision][0], f * self.yard[precision][1]


@pytest.fixture(scope="module")
def cases(need_gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(name)
        return made[name]

    yield get
    for c in made.values():
        for g in c._gpu.values():
            g.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_hidden_state_vs_f64(cases, name, precision):
    c = cases(name)
    hid = c.hidden(precision)
    assert hid.shape == c.ref.shape and hid.dtype == torch.float32
    assert bool(torch.isfinite(hid).all())
    rms, worst = R.rel_rms(hid, c.ref), R.worst_token(hid, c.ref)
    y_rms, y_worst = c.yard[precision]
    print(f"[{name} {precision}] rel RMS {rms:.3e} (yardstick {y_rms:.3e}, ratio {rms / y_rms:.2f}); "
          f"worst token {worst:.3e} (yardstick {y_worst:.3e}, ratio {worst / y_worst:.2f})")
    b_rms, b_worst = c.bound(precision)
    assert rms <= b_rms
    assert worst <= b_worst


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_pooling_of_own_hidden_state(cases, name, precision):
    """cls and max are copies and comparisons: bit-equal to the same
    operation on the GPU's own hidden state (max over all S positions, padded
    ones included). mean is k_pool's sequential f32 sum of S terms: within
    S * 2^-23 * max|hidden| of the float64 mean over the mask."""
    c = cases(name)
    g, hid = c.gpu(precision), c.hidden(precision)
    S = c.ids.shape[1]
    for mode in ("cls", "max"):
        got = g.forward(c.ids, c.mask, c.tt, pooling=mode).cpu()
        assert got.shape == (c.ids.shape[0], c.cfg["hidden_size"])
        assert torch.equal(got, R.pool(hid, c.mask, mode)), mode
    got = g.forward(c.ids, c.mask, c.tt, pooling="mean").cpu().double()
    err = float((got - R.pool(hid.double(), c.mask, "mean")).abs().max())
    bound = S * 2.0 ** -23 * float(hid.abs().max())
    print(f"[{name} {precision}] mean pooling: max |diff| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["s65", "s257", "s200"])
def test_sequence_does_not_depend_on_its_batch(cases, name, precision):
    """Masked keys and the other rows of a batch contribute nothing: each row
    run alone (cut to its valid length where its mask is a prefix) agrees
    with the same row inside the batch over its valid positions, and in its
    mean pooling, within the case's bound of test_hidden_state_vs_f64."""
    c = cases(name)
    g, hid = c.gpu(precision), c.hidden(precision)
    pooled = g.forward(c.ids, c.mask, c.tt, pooling="mean").cpu()
    b_rms, b_worst = c.bound(precision)
    for b in range(c.ids.shape[0]):
        n = int(c.mask[b].sum())
        prefix = bool((c.mask[b, :n] == 1).all())
        cut = n if prefix else c.ids.shape[1]
        args = (c.ids[b:b + 1, :cut], c.mask[b:b + 1, :cut], c.tt[b:b + 1, :cut])
        alone = g.forward(*args, pooling="none").cpu()[0]
        valid = c.mask[b, :cut].bool()
        rms, worst = R.rel_rms(alone[valid], hid[b, :cut][valid]), R.worst_token(alone[valid], hid[b, :cut][valid])
        pm = R.rel_rms(g.forward(*args, pooling="mean").cpu()[0], pooled[b])
        print(f"[{name} {precision}] row {b} ({n} of {cut} tokens) alone vs in its batch: rel RMS {rms:.3e}, "
              f"worst token {worst:.3e}, mean pooling {pm:.3e}")
        assert rms <= b_rms and worst <= b_worst and pm <= b_rms, b


@pytest.mark.parametrize("precision", PRECISIONS)
def test_workspace_reuse_and_determinism(cases, precision):
    """One handle serves calls of different B and S from one workspace (grown,
    then reused at a smaller size, then at the larger again); each result is
    bit-equal to a fresh handle's, and a repeated call to itself: the forward
    has no atomics and reads nothing a former call left behind."""
    from fheicp.bert import GpuBert
    big, small = cases("s200"), cases("s65")       # both H = 128; the weights are s65's (two layers)
    assert big.cfg["hidden_size"] == small.cfg["hidden_size"] == 128
    run = lambda g, c: g.forward(c.ids, c.mask, c.tt, pooling="none").cpu()
    g = small.gpu(precision)
    seq = [run(g, big), run(g, small), run(g, big), run(g, big)]
    for c, outs in ((big, (seq[0], seq[2], seq[3])), (small, (seq[1],))):
        fresh = GpuBert(state_dict=small.sd, config=small.cfg, device=0, precision=precision)
        want = run(fresh, c)
        fresh.close()
        assert bool(torch.isfinite(want).all())
        for i, o in enumerate(outs):
            assert torch.equal(o, want), (c.name, i)


def _raw_handle(cfg, sd, skip=None):
    """a handle through the C ABI with every tensor of sd but `skip` loaded"""
    from fheicp import _lib
    from fheicp.bert import _EMB, _LAYER, BertConfigC, _cfg_dict
    L = _lib.lib()
    h = C.c_void_p()
    assert L.fhe_bert_create(C.byref(BertConfigC(**_cfg_dict(cfg))), 0, C.byref(h)) == 0
    for name, t in sd.items():
        if name == skip:
            continue
        a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
        if name in _EMB:
            layer, which = -1, _EMB[name]
        else:
            li, _, sub = name[len("encoder.layer."):].partition(".")
            layer, which = int(li), _LAYER[sub]
        assert L.fhe_bert_set_tensor(h, layer, which, C.c_void_p(a.ctypes.data), a.size) == 0, name
    return L, h


def test_forward_argument_checks(cases):
    """fhe_bert_forward refuses what include/fhe_bert.h excludes before any
    launch, and GpuBert.forward what the ABI cannot see (ids, types and the
    first key of each row). No kernel runs with a masked first key."""
    c = cases("s1")
    H, maxpos = c.cfg["hidden_size"], c.cfg["max_position_embeddings"]
    L, h = _raw_handle(c.cfg, c.sd)
    dev = torch.device("cuda", 0)
    n = maxpos + 1                                  # room for every call below, had it run
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    mask = torch.ones(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n * H, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    fwd = lambda hh, i, m, o, B, S, pooling: L.fhe_bert_forward(hh, i, None, m, B, S, pooling, o, None)
    try:
        assert L.fhe_bert_ready(h) == 1
        assert fwd(h, p(ids), p(mask), p(out), 1, 0, 3) == E_ARG
        assert fwd(h, p(ids), p(mask), p(out), 1, maxpos + 1, 3) == E_ARG
        assert fwd(h, p(ids), p(mask), p(out), 1, 1, 4) == E_ARG
        assert fwd(h, p(ids), p(mask), p(out), 1, 1, -1) == E_ARG
        assert fwd(h, p(ids), p(mask), p(out), -1, 1, 3) == E_ARG
        assert fwd(h, None, p(mask), p(out), 1, 1, 3) == E_ARG
        assert fwd(h, p(ids), None, p(out), 1, 1, 3) == E_ARG
        assert fwd(h, p(ids), p(mask), None, 1, 1, 3) == E_ARG
        assert fwd(h, None, None, None, 0, 1, 3) == 0
        a = np.zeros(H + 1, np.float32)
        assert L.fhe_bert_set_tensor(h, 0, 17, C.c_void_p(a.ctypes.data), a.size) == E_ARG    # FHE_BERT_Q_B
        msg = L.fhe_bert_last_error(h).decode()
        assert str(H + 1) in msg and str(H) in msg, msg
        assert fwd(h, p(ids), p(mask), p(out), 1, 1, 3) == 0         # the handle still works
        torch.cuda.synchronize()
    finally:
        L.fhe_bert_destroy(h)
    L, h = _raw_handle(c.cfg, c.sd, skip="encoder.layer.0.output.dense.bias")
    try:
        assert L.fhe_bert_ready(h) == 0
        assert fwd(h, p(ids), p(mask), p(out), 1, 1, 3) == E_STATE
    finally:
        L.fhe_bert_destroy(h)

    c = cases("s65")
    g = c.gpu("f32")
    bad = c.mask.clone()
    bad[2, 0] = 0
    with pytest.raises(ValueError):
        g.forward(c.ids, bad, c.tt)
    for v in (R.VOCAB, -1):
        bad = c.ids.clone()
        bad[1, 3] = v
        with pytest.raises(ValueError):
            g.forward(bad, c.mask, c.tt)
    for v in (2, -1):
        bad = c.tt.clone()
        bad[4, 64] = v
        with pytest.raises(ValueError):
            g.forward(c.ids, c.mask, bad)
    with pytest.raises(ValueError):
        g.forward(c.ids, c.mask[:, :-1], c.tt)
    with pytest.raises(ValueError):
        g.forward(c.ids, c.mask, c.tt[:, :-1])
    with pytest.raises(ValueError):
        g.forward(c.ids[0], c.mask[0], c.tt[0])
    with pytest.raises(ValueError):
        g.forward(c.ids, c.mask, c.tt, pooling="median")
