"""Plain torch restatement of the encoder (include/fhe_bert.h) on the CPU,
shared by tests/test_bert_ref_cpu.py (which pins it against transformers'
BertModel in float64) and tests/test_gpu_bert_edges.py (which compares
libfheicp's encoder against it in float64). No transformers import here.

The weights are drawn so that no term is trivial (biases, LayerNorm gains and
shifts all non-zero; attention logits of std 2 to 3 so the softmax is far from
uniform), and the cases are the shapes at which the kernels of
fhe-icp_amd/csrc/bert.hip change path."""
import math

import torch

VOCAB = 97

# id -> H, I, layers, B, S, valid lengths (what each reaches: docs/AB_LOG_r10.md)
CASES = {
    "s1": dict(H=64, I=64, L=1, B=3, S=1, lens=(1, 1, 1)),
    "s65": dict(H=128, I=192, L=2, B=5, S=65, lens=(65, 1, 64, 33, 2)),   # + holes in row 0
    "s129": dict(H=256, I=320, L=2, B=3, S=129, lens=(129, 128, 65)),
    "s257": dict(H=192, I=448, L=1, B=2, S=257, lens=(257, 70)),
    "s512": dict(H=128, I=128, L=1, B=1, S=512, lens=(512,)),
    "s200": dict(H=128, I=192, L=1, B=4, S=200, lens=(200, 64, 1, 63)),
    "h1024": dict(H=1024, I=64, L=1, B=1, S=40, lens=(40,)),
    "h960": dict(H=960, I=128, L=1, B=2, S=9, lens=(9, 3)),
    "base1": dict(H=768, I=3072, L=1, B=2, S=100, lens=(100, 37)),
}


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def make_weights(H, I, L, vocab=VOCAB, seed=0):
    """(config dict, float32 state dict under the HF BertModel names)."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    cfg = {"vocab_size": vocab, "hidden_size": H, "num_hidden_layers": L, "num_attention_heads": H // 64,
           "intermediate_size": I, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12,
           "hidden_act": "gelu"}
    sd = {}

    def ln(name):
        sd[name + ".weight"] = 1 + 0.3 * n(H)
        sd[name + ".bias"] = 0.3 * n(H)

    def lin(name, out, inp, var):
        sd[name + ".weight"] = math.sqrt(var) * n(out, inp)
        sd[name + ".bias"] = 0.3 * n(out)

    sd["embeddings.word_embeddings.weight"] = n(vocab, H)
    sd["embeddings.position_embeddings.weight"] = n(512, H)
    sd["embeddings.token_type_embeddings.weight"] = n(2, H)
    ln("embeddings.LayerNorm")
    for l in range(L):
        p = f"encoder.layer.{l}."
        lin(p + "attention.self.query", H, H, 2.0 / H)
        lin(p + "attention.self.key", H, H, 2.0 / H)
        lin(p + "attention.self.value", H, H, 1.0 / H)
        lin(p + "attention.output.dense", H, H, 1.0 / H)
        ln(p + "attention.output.LayerNorm")
        lin(p + "intermediate.dense", I, H, 1.0 / H)
        lin(p + "output.dense", H, I, 1.0 / I)
        ln(p + "output.LayerNorm")
    return cfg, sd


def case_weights(name):
    """make_weights for a case of CASES, seeded by its place in the table
    (from 2: under seeds 0 and 1 the three logits of s1 happen to lie close
    together, and test_bert_ref_cpu.py asks every case for a spread >= 1)"""
    c = CASES[name]
    return make_weights(c["H"], c["I"], c["L"], VOCAB, seed=2 + list(CASES).index(name))


def make_inputs(name, seed=0):
    """ids, mask, token types (int64 [B][S]) of a case: ids 0 and VOCAB - 1
    both occur, token types are random, every row has mask[b][0] = 1."""
    c = CASES[name]
    B, S = c["B"], c["S"]
    g = torch.Generator().manual_seed(1000 + seed)
    ids = torch.randint(0, VOCAB, (B, S), generator=g)
    ids[0, 0] = 0
    if S > 1:
        ids[0, S - 1] = VOCAB - 1
    else:
        ids[1, 0] = VOCAB - 1
    tt = torch.randint(0, 2, (B, S), generator=g)
    mask = (torch.arange(S)[None, :] < torch.tensor(c["lens"])[:, None]).to(torch.int64)
    if name == "s65":
        mask[0, 5:60:3] = 0
    return ids, mask, tt


def _layernorm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)      # biased
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _embed(W, cfg, ids, tt):
    S = ids.shape[1]
    e = (W["embeddings.word_embeddings.weight"][ids] + W["embeddings.position_embeddings.weight"][:S][None]
         + W["embeddings.token_type_embeddings.weight"][tt])
    return _layernorm(e, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], cfg["layer_norm_eps"])


def _heads(x, nh):
    B, S, H = x.shape
    return x.view(B, S, nh, H // nh).transpose(1, 2)       # [B][nh][S][64]


def forward(sd, cfg, ids, mask, tt, dtype=torch.float64, rnd=None, logits=None):
    """last_hidden_state [B][S][H] in `dtype`. `rnd` (e.g. bf16) is applied
    where FHE_BERT_BF16 rounds: the four GEMM weights, each GEMM's activation
    input, the Q/K/V outputs, the softmax probabilities, the context and the
    GELU output; the residual stream, biases and LayerNorm stay unrounded.
    `logits`, a list, receives each layer's scaled scores before the mask."""
    r = rnd if rnd is not None else (lambda x: x)
    W = {k: v.to(dtype) for k, v in sd.items()}
    nh, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    B, S = ids.shape
    h = _embed(W, cfg, ids, tt)
    neg = torch.zeros(B, 1, 1, S, dtype=dtype).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    lin = lambda x, name: r(x) @ r(W[name + ".weight"]).T + W[name + ".bias"]
    for l in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{l}."
        q, k, v = (_heads(r(lin(h, p + "attention.self." + n)), nh) for n in ("query", "key", "value"))
        s = q @ k.transpose(-1, -2) * 0.125
        if logits is not None:
            logits.append(s)
        pr = r(torch.softmax(s + neg, dim=-1))
        ctx = r((pr @ v).transpose(1, 2).reshape(B, S, -1))
        h = _layernorm(lin(ctx, p + "attention.output.dense") + h, W[p + "attention.output.LayerNorm.weight"],
                       W[p + "attention.output.LayerNorm.bias"], eps)
        x = lin(h, p + "intermediate.dense")
        x = r(0.5 * x * (1 + torch.erf(x / math.sqrt(2.0))))
        h = _layernorm(lin(x, p + "output.dense") + h, W[p + "output.LayerNorm.weight"],
                       W[p + "output.LayerNorm.bias"], eps)
    return h


def pool(hid, mask, mode):
    """bert_embeddings.py's pooling: mean over the mask, [CLS], or max over
    all S positions (padded ones included), in the dtype of `hid`."""
    if mode == "mean":
        am = mask.unsqueeze(-1).to(hid.dtype)
        return (hid * am).sum(1) / am.sum(1)
    if mode == "cls":
        return hid[:, 0, :]
    return hid.max(dim=1)[0]


def rel_rms(x, ref):
    """relative RMS error of the whole tensor, in float64"""
    x, ref = x.double(), ref.double()
    return float(((x - ref) ** 2).sum().sqrt() / (ref ** 2).sum().sqrt())


def worst_token(x, ref):
    """the largest relative RMS error of one token's row [..., H]"""
    x, ref = x.double(), ref.double()
    return float((((x - ref) ** 2).sum(-1).sqrt() / (ref ** 2).sum(-1).sqrt()).max())
