"""CPU: pins tests/bert_ref.py, the restatement tests/test_gpu_bert_edges.py
compares libfheicp's encoder against, to transformers' BertModel in float64
on every case of bert_ref.CASES, over all positions (padded ones included),
and asserts the two conditions on the inputs that the GPU tests rely on: the
softmax is far from uniform (layer-0 logits of std >= 1) and every row keeps
its first key. The restatement's own float32 and bf16-rounded errors against
float64 (the yardsticks of the GPU test) are printed, not asserted."""
import pytest
import torch

import bert_ref as R


@pytest.fixture(scope="module", params=list(R.CASES))
def case(request):
    cfg, sd = R.case_weights(request.param)
    ids, mask, tt = R.make_inputs(request.param)
    logits = []
    ref = R.forward(sd, cfg, ids, mask, tt, logits=logits)
    return request.param, cfg, sd, ids, mask, tt, ref, logits


def test_restatement_equals_transformers_f64(case):
    from transformers import BertConfig, BertModel
    name, cfg, sd, ids, mask, tt, ref, _ = case
    m = BertModel(BertConfig(**cfg), add_pooling_layer=False).eval()
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        want = m.double()(input_ids=ids, attention_mask=mask, token_type_ids=tt).last_hidden_state
    assert want.dtype == torch.float64 and ref.dtype == torch.float64 and ref.shape == want.shape
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(want).all())
    e = R.rel_rms(ref, want)
    print(f"[{name}] restatement vs transformers f64, all positions: rel RMS {e:.2e}")
    assert e <= 1e-12


def test_inputs_keep_the_softmax_sharp_and_the_first_key(case):
    name, cfg, sd, ids, mask, tt, _, logits = case
    c = R.CASES[name]
    assert ids.shape == mask.shape == tt.shape == (c["B"], c["S"])
    assert bool((mask[:, 0] == 1).all())
    assert tuple(int(x) for x in mask.sum(1)) == tuple(
        n - (len(range(5, 60, 3)) if (name, b) == ("s65", 0) else 0) for b, n in enumerate(c["lens"]))
    assert int(ids.min()) == 0 and int(ids.max()) == R.VOCAB - 1
    assert set(tt.unique().tolist()) <= {0, 1}
    std = float(logits[0].std())
    print(f"[{name}] layer-0 logits: std {std:.2f}")
    assert std >= 1.0
    if c["S"] > 1:      # and over the keys of one softmax row, which is what sharpens it
        row = float(logits[0].std(dim=-1).mean())
        print(f"[{name}] layer-0 logits: mean std over the keys of a row {row:.2f}")
        assert row >= 1.0


def test_print_yardsticks(case):
    name, cfg, sd, ids, mask, tt, ref, _ = case
    f32 = R.forward(sd, cfg, ids, mask, tt, dtype=torch.float32)
    b16 = R.forward(sd, cfg, ids, mask, tt, rnd=R.bf16)
    assert f32.dtype == torch.float32 and bool(torch.isfinite(f32).all()) and bool(torch.isfinite(b16).all())
    print(f"[{name}] float32 restatement vs f64: rel RMS {R.rel_rms(f32, ref):.2e}, worst token "
          f"{R.worst_token(f32, ref):.2e}; bf16-rounded: rel RMS {R.rel_rms(b16, ref):.2e}, worst token "
          f"{R.worst_token(b16, ref):.2e}")
