"""Plain-torch fp32 restatement of GroundingDINO's text side over a state dict — test infrastructure: transformers' BertModel (the sum of three
embeddings, LayerNorm, post-LN layers, erf-GELU, logits scaled by d^-0.5 with disallowed keys at -inf, a tanh pooler on row 0), `feat_map`, and
a vectorised restatement of the sub-sentence rule of the reference's bertwarper.py:180-273 (spans, position ids, dense mask, cate_to_token
masks).  The CPU suite pins it to tests/golden/bert_tiny_*.npz (which transformers and the reference's own functions produced); the GPU suite
trusts it at sizes the fixture cannot hold.

`bf16_storage=True` gives the CONTROL of the project's standing tolerance rule (tests/clip_ref.py's convention): fp32 arithmetic, matrix
weights and embedding tables rounded to bf16 (what the module packs), and every activation rounded to bf16 exactly where the HIP path stores
one in HBM.  Each `_st(...)` below is one `# bf16:` mark of anyedit_amd/groundingdino/bertwarper.py (BertModel.forward) and
groundingdino.py (encode_tokenized); keep the lists in step.  The intermediate product and the pooler are NOT rounded: they stay fp32.
"""
import torch
import torch.nn.functional as F


def _round(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---- the sub-sentence rule -------------------------------------------------------------------------------------------------------------------
def special_mask(ids, special_ids):
    ids = torch.as_tensor(ids).long()
    s = torch.zeros_like(ids, dtype=torch.bool)
    for t in special_ids:
        s |= ids == int(t)
    return s


def text_spans(ids, special_ids):
    """ids [B, N] -> (spans int64 [B, N, 2] = (lo, hi), position_ids int64 [B, N]).  With e the first special position >= n and p the last
    special position before e: e exists, e != 0, e != N-1 -> [p+1, e+1), position n - (p+1); otherwise [n, n+1), position 0."""
    s = special_mask(ids, special_ids)
    B, N = s.shape
    ar = torch.arange(N).expand(B, N)
    nxt = torch.where(s, ar, torch.full_like(ar, N)).flip(1).cummin(1).values.flip(1)            # first special >= n (N: none)
    last = torch.where(s, ar, torch.full_like(ar, -1)).cummax(1).values                          # last special <= n (-1: none)
    last_before = torch.cat([torch.full((B, 1), -1, dtype=torch.long), last[:, :-1]], 1)         # last special < n
    e = nxt.clamp(max=N - 1)
    p = last_before.gather(1, e)                                                                 # last special before e
    phrase = (nxt < N) & (nxt != 0) & (nxt != N - 1)
    lo = torch.where(phrase, p + 1, ar)
    hi = torch.where(phrase, nxt + 1, ar + 1)
    return torch.stack([lo, hi], -1), ar - lo


def spans_to_mask(spans):
    """[B, N, 2] -> bool [B, N, N]: key k is allowed for query n when lo <= k < hi."""
    N = spans.shape[1]
    k = torch.arange(N).view(1, 1, N)
    return (k >= spans[..., :1]) & (k < spans[..., 1:])


def cate_to_token(ids, special_ids):
    """bertwarper.py:259-261: per sample a bool [phrases, N] tensor, one row per special token that is neither first nor last."""
    s = special_mask(ids, special_ids)
    spans, _ = text_spans(ids, special_ids)
    B, N = s.shape
    out = []
    for b in range(B):
        rows = []
        for e in torch.nonzero(s[b]).flatten().tolist():
            if e in (0, N - 1):
                continue
            r = torch.zeros(N, dtype=torch.bool)
            r[int(spans[b, e, 0]):e] = True
            rows.append(r)
        out.append(torch.stack(rows, 0) if rows else torch.zeros(0, N, dtype=torch.bool))
    return out


# ---- BertModel ------------------------------------------------------------------------------------------------------------------------------
def bert_forward(sd, ids, heads, allowed=None, position_ids=None, token_type_ids=None, eps=1e-12, bf16_storage=False, prefix=""):
    """sd: Hugging Face BertModel state dict under `prefix`; ids [B, N]; allowed: None (every key), bool [B, N] (keys) or bool [B, N, N]
    (query, key).  Returns dict(hidden_states=[L + 1 tensors], last_hidden_state, pooler_output)."""
    _st = _round if bf16_storage else (lambda t: t)
    w = (lambda k: _round(sd[prefix + k].float())) if bf16_storage else (lambda k: sd[prefix + k].float())   # bf16 weight images / tables
    f = lambda k: sd[prefix + k].float()                                                                        # fp32 biases / affine vectors
    ids = torch.as_tensor(ids).long()
    B, N = ids.shape
    pos = torch.arange(N).expand(B, N) if position_ids is None else torch.as_tensor(position_ids).long()
    typ = torch.zeros(B, N, dtype=torch.long) if token_type_ids is None else torch.as_tensor(token_type_ids).long()
    e = w("embeddings.word_embeddings.weight")[ids] + w("embeddings.position_embeddings.weight")[pos] + w("embeddings.token_type_embeddings.weight")[typ]
    C = e.shape[-1]
    x = _st(F.layer_norm(e, (C,), f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias"), eps))     # bf16: embeddings after their LayerNorm
    d = C // heads
    L = 0
    while prefix + f"encoder.layer.{L}.attention.self.query.weight" in sd:
        L += 1
    bias = torch.zeros(B, 1, N, N)
    if allowed is not None:
        a = torch.as_tensor(allowed).bool()
        a = a.view(B, 1, 1, N) if a.dim() == 2 else a.view(B, 1, N, N)
        bias = torch.zeros(B, 1, N, N).masked_fill(~a.expand(B, 1, N, N), float("-inf"))
    sp = lambda t: t.view(B, N, heads, d).transpose(1, 2)
    hs = [x]
    for i in range(L):
        q = f"encoder.layer.{i}."
        wqkv = torch.cat([w(q + f"attention.self.{n}.weight") for n in ("query", "key", "value")], 0)
        bqkv = torch.cat([f(q + f"attention.self.{n}.bias") for n in ("query", "key", "value")], 0)
        qq, kk, vv = _st(F.linear(x, wqkv, bqkv)).split(C, dim=-1)                                              # bf16: packed q | k | v
        a = (sp(qq) @ sp(kk).transpose(-1, -2)) * d ** -0.5 + bias
        o = _st((a.softmax(-1) @ sp(vv)).transpose(1, 2).reshape(B, N, C))                                      # bf16: attention output
        m = _st(x + F.linear(o, w(q + "attention.output.dense.weight"), f(q + "attention.output.dense.bias")))  # bf16: x + attention projection
        y = _st(F.layer_norm(m, (C,), f(q + "attention.output.LayerNorm.weight"), f(q + "attention.output.LayerNorm.bias"), eps))   # bf16: attention.output.LayerNorm
        u = F.linear(y, w(q + "intermediate.dense.weight"), f(q + "intermediate.dense.bias"))                   # fp32: intermediate product + bias
        u = _st(F.gelu(u))                                                                                      # bf16: activated hidden values
        m = _st(y + F.linear(u, w(q + "output.dense.weight"), f(q + "output.dense.bias")))                      # bf16: y + output projection
        x = _st(F.layer_norm(m, (C,), f(q + "output.LayerNorm.weight"), f(q + "output.LayerNorm.bias"), eps))   # bf16: output.LayerNorm = hidden_states[i + 1]
        hs.append(x)
    pooled = torch.tanh(F.linear(x[:, 0], w("pooler.dense.weight"), f("pooler.dense.bias")))                   # fp32: pooler_output
    return dict(hidden_states=hs, last_hidden_state=x, pooler_output=pooled)


def feat_map(sd, x, bf16_storage=False, prefix="feat_map."):
    wt = sd[prefix + "weight"].float()
    y = F.linear(x, _round(wt) if bf16_storage else wt, sd[prefix + "bias"].float())
    return _round(y) if bf16_storage else y                                                                     # bf16: feat_map


def seeded_state_dict(cfg, hidden_dim=256, seed=0):
    """Seeded weights of a `GroundingDINOText` of geometry `cfg` (keys `bert.*`, `feat_map.*`), for sizes no fixture can hold: embeddings
    N(0, 0.05^2), matrices U(-a, a) with a = sqrt(3 / fan_in) (q / k x 2 so that the logits are not degenerate), LayerNorm weights U(0.5, 1.5),
    every bias N(0, 0.1^2); every tensor rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    C, I, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    n = lambda *s, std: torch.randn(*s, generator=g) * std
    u = lambda o, i, k=1.0: (2 * torch.rand(o, i, generator=g) - 1) * (3.0 / i) ** 0.5 * k
    sd = {}

    def lin(name, o, i, k=1.0):
        sd[name + ".weight"], sd[name + ".bias"] = u(o, i, k), n(o, std=0.1)

    def ln(name):
        sd[name + ".weight"], sd[name + ".bias"] = 0.5 + torch.rand(C, generator=g), n(C, std=0.1)

    sd["embeddings.word_embeddings.weight"] = n(cfg["vocab_size"], C, std=0.05)
    sd["embeddings.position_embeddings.weight"] = n(cfg["max_position_embeddings"], C, std=0.05)
    sd["embeddings.token_type_embeddings.weight"] = n(cfg["type_vocab_size"], C, std=0.05)
    ln("embeddings.LayerNorm")
    for i in range(L):
        q = f"encoder.layer.{i}."
        lin(q + "attention.self.query", C, C, 2.0)
        lin(q + "attention.self.key", C, C, 2.0)
        lin(q + "attention.self.value", C, C)
        lin(q + "attention.output.dense", C, C)
        ln(q + "attention.output.LayerNorm")
        lin(q + "intermediate.dense", I, C)
        lin(q + "output.dense", C, I)
        ln(q + "output.LayerNorm")
    lin("pooler.dense", C, C)
    sd = {"bert." + k: v for k, v in sd.items()}
    sd["feat_map.weight"], sd["feat_map.bias"] = u(hidden_dim, C), n(hidden_dim, std=0.1)
    return {k: _round(v) for k, v in sd.items()}


# ---- the fixtures (tests/golden/bert_tiny_*.npz, tools/gen_golden_bert.py) -------------------------------------------------------------------
GEOMS = ("a", "b")
_CACHE = {}


def stored(geom):
    """bert_tiny_<geom>_io.npz as a dict of numpy arrays (cached; treat as read-only)."""
    from conftest import load_golden
    if ("io", geom) not in _CACHE:
        _CACHE["io", geom] = load_golden(f"bert_tiny_{geom}_io")
    return _CACHE["io", geom]


def weights(geom):
    """The fixture's state dict (`bert.*`, `feat_map.*`) as fp32 tensors holding bf16 values (cached; treat as read-only)."""
    import os
    import numpy as np
    from conftest import GOLDEN, load_golden
    if ("w", geom) not in _CACHE:
        sd, i = {}, 0
        while os.path.exists(os.path.join(GOLDEN, f"bert_tiny_{geom}_w{i}.npz")):
            for k, v in load_golden(f"bert_tiny_{geom}_w{i}").items():
                sd[k[2:]] = torch.from_numpy(np.ascontiguousarray(v)).view(torch.bfloat16).float()
            i += 1
        assert sorted(sd) == [str(k) for k in stored(geom)["keys"]], "every slice of the state dict was found"
        _CACHE["w", geom] = sd
    return _CACHE["w", geom]


def config(geom):
    return {k[len("config."):]: int(v) for k, v in stored(geom).items() if k.startswith("config.")}


def module(geom, device="cpu", **kw):
    """A `GroundingDINOText` of the fixture's geometry with the fixture's weights, in eval mode."""
    from anyedit_amd.checkpoints import load_groundingdino_text
    from anyedit_amd.groundingdino.groundingdino import GroundingDINOText
    cfg = config(geom)
    hidden_dim = cfg.pop("hidden_dim")
    m = GroundingDINOText(cfg, hidden_dim=hidden_dim, special_token_ids=[int(t) for t in stored(geom)["special_ids"]], **kw)
    load_groundingdino_text(m, dict(weights(geom)))
    return m.eval().requires_grad_(False).to(device)
