"""Plain-torch fp32 restatement of the CLIP text tower (transformers' CLIPTextModel: embeddings, pre-LN causal layers, final LayerNorm,
pooled row at the first EOS) over a state dict — test infrastructure: the CPU suite pins it to tests/golden/clip_text_tiny.npz (which
transformers itself produced), the GPU suite trusts it at sizes the fixture cannot hold.

`bf16_storage=True` gives the CONTROL of the project's standing tolerance rule (oracle/ldm_ref.py's `_st` / `bf16_storage()` /
`bf16_weights` convention): fp32 arithmetic, matrix weights and embedding tables rounded to bf16 (what the module packs), and every
activation rounded to bf16 exactly where the HIP path stores one in HBM.  Each `_st(...)` below is one `# bf16:` mark of
anyedit_amd/ldm/modules/encoders/modules.py (CLIPTextTower.run / final_norm); keep the two lists in step.  The LayerNorm outputs ARE
rounded: the library's LayerNorm fold covers K = 320 only, so the tower's LayerNorms are launches of their own that store bf16 rows.
The fc1 product is NOT rounded: bias and activation are applied to the fp32 product.
"""
import torch
import torch.nn.functional as F

PREFIX = "transformer.text_model."


def _round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def clip_text_forward(sd, ids, heads, act="quick_gelu", eps=1e-5, eos_token_id=None, bf16_storage=False, prefix=PREFIX, n_layers=None):
    """sd: state dict with `prefix` keys; ids [B, N] int.  Returns dict(hidden_states=[L + 1 tensors, no final LayerNorm], last_hidden_state,
    pooler_output (when eos_token_id is given), final_norm=callable applying the final LayerNorm to any hidden state)."""
    _st = _round if bf16_storage else (lambda t: t)
    w = (lambda k: _round(sd[prefix + k].float())) if bf16_storage else (lambda k: sd[prefix + k].float())   # bf16 weight images
    f = lambda k: sd[prefix + k].float()                                                                        # fp32 biases / affine vectors
    ids = torch.as_tensor(ids).long()
    B, N = ids.shape
    x = _st(w("embeddings.token_embedding.weight")[ids] + w("embeddings.position_embedding.weight")[:N])       # bf16: embedding sum
    C = x.shape[-1]
    d = C // heads
    L = 0
    while prefix + f"encoder.layers.{L}.layer_norm1.weight" in sd:
        L += 1
    mask = torch.full((N, N), float("-inf")).triu(1)
    sp = lambda t: t.view(B, N, heads, d).transpose(1, 2)
    hs = [x]
    for i in range(L if n_layers is None else n_layers):
        q = f"encoder.layers.{i}."
        h = _st(F.layer_norm(x, (C,), f(q + "layer_norm1.weight"), f(q + "layer_norm1.bias"), eps))            # bf16: LayerNorm1 output
        wqkv = torch.cat([w(q + f"self_attn.{n}_proj.weight") for n in "qkv"], 0)
        bqkv = torch.cat([f(q + f"self_attn.{n}_proj.bias") for n in "qkv"], 0)
        qq, kk, vv = _st(F.linear(h, wqkv, bqkv)).split(C, dim=-1)                                              # bf16: packed q | k | v
        a = (sp(qq) @ sp(kk).transpose(-1, -2)) * d ** -0.5 + mask
        o = _st((a.softmax(-1) @ sp(vv)).transpose(1, 2).reshape(B, N, C))                                      # bf16: attention output
        x = _st(x + F.linear(o, w(q + "self_attn.out_proj.weight"), f(q + "self_attn.out_proj.bias")))          # bf16: residual stream after the attention add
        h = _st(F.layer_norm(x, (C,), f(q + "layer_norm2.weight"), f(q + "layer_norm2.bias"), eps))            # bf16: LayerNorm2 output
        u = F.linear(h, w(q + "mlp.fc1.weight"), f(q + "mlp.fc1.bias"))                                         # fp32: fc1 product + bias
        u = _st(u * torch.sigmoid(1.702 * u) if act == "quick_gelu" else F.gelu(u))                             # bf16: activated hidden values
        x = _st(x + F.linear(u, w(q + "mlp.fc2.weight"), f(q + "mlp.fc2.bias")))                                # bf16: residual stream after the MLP add
        hs.append(x)
    fin = lambda t: _st(F.layer_norm(t, (C,), f("final_layer_norm.weight"), f("final_layer_norm.bias"), eps))  # bf16: final LayerNorm output
    out = dict(hidden_states=hs, final_norm=fin, last_hidden_state=fin(hs[-1]))
    if eos_token_id is not None:
        pos = (ids == eos_token_id).int().argmax(-1)
        out["pooler_output"] = out["last_hidden_state"][torch.arange(B), pos]
    return out


def hacked_forward(sd, tokens, heads, clip_skip=0, **kw):
    """cldm/hack.py:40-45, 62-68 over framed ids [B, 3, 77]: [B, 231, C]; clip_skip > 1 -> final_layer_norm(hidden_states[-clip_skip])."""
    t = torch.as_tensor(tokens).long()
    B, Fr, N = t.shape
    r = clip_text_forward(sd, t.reshape(B * Fr, N), heads, **kw)
    y = r["final_norm"](r["hidden_states"][-clip_skip]) if clip_skip > 1 else r["last_hidden_state"]
    return y.reshape(B, Fr * N, -1)


def seeded_state_dict(cfg, seed=0, prefix=PREFIX):
    """Seeded weights of a tower of geometry `cfg` (the keys of FrozenCLIPEmbedder.state_dict()), for sizes no fixture can hold: the init
    transformers gives CLIPTextModel (embeddings N(0, 0.02); q/k/v std C^-0.5 (2L)^-0.5, out_proj and fc2 C^-0.5 resp. (2C)^-0.5 scaled the same
    way, fc1 (2C)^-0.5; LayerNorm 1 / 0) with the fixture generator's rescaling (matrix weights x 3, biases N(0, 0.1)) so that the logits are
    not degenerate, every tensor rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    C, I, L, V, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["vocab_size"], cfg["max_position_embeddings"]
    n = lambda *s, std: torch.randn(*s, generator=g) * std
    in_std, out_std, fc_std = C ** -0.5 * (2 * L) ** -0.5, C ** -0.5, (2 * C) ** -0.5
    sd = {"embeddings.token_embedding.weight": n(V, C, std=0.02), "embeddings.position_embedding.weight": n(P, C, std=0.02),
          "final_layer_norm.weight": torch.ones(C), "final_layer_norm.bias": n(C, std=0.1)}
    for i in range(L):
        q = f"encoder.layers.{i}."
        for name, shape, std in (("self_attn.q_proj", (C, C), in_std), ("self_attn.k_proj", (C, C), in_std), ("self_attn.v_proj", (C, C), in_std),
                                 ("self_attn.out_proj", (C, C), out_std), ("mlp.fc1", (I, C), fc_std), ("mlp.fc2", (C, I), in_std)):
            sd[q + name + ".weight"] = n(*shape, std=3.0 * std)
            sd[q + name + ".bias"] = n(shape[0], std=0.1)
        for name in ("layer_norm1", "layer_norm2"):
            sd[q + name + ".weight"] = torch.ones(C)
            sd[q + name + ".bias"] = n(C, std=0.1)
    return {prefix + k: _round(v) for k, v in sd.items()}
