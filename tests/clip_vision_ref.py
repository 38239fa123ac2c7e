"""Plain-torch fp32 restatement of the CLIP vision tower (transformers' CLIPVisionModelWithProjection: patch convolution, class + position
embeddings, pre_layrnorm, pre-LN layers with full attention, post_layernorm of the class row, visual projection) over a state dict — test
infrastructure: the CPU suite pins it to tests/golden/clip_vision_tiny*.npz (which transformers itself produced), the GPU suite trusts it
at sizes the fixtures cannot hold.

`bf16_storage=True` gives the CONTROL of the project's standing tolerance rule (tests/clip_ref.py's convention): fp32 arithmetic, matrix
weights rounded to bf16 (what the module packs: patch embedding, the six projections of a layer, the visual projection) and every
activation rounded to bf16 exactly where the HIP path stores one in HBM.  Each `_st(...)` below is one `# bf16:` mark of
anyedit_amd/ldm/modules/encoders/clip_vision.py (run / forward); keep the two lists in step.  NOT rounded: the class and position
embeddings (fp32 on the HIP path, added to the fp32 patch product), the patch product and its un-normalised sum, the fc1 product.
"""
import torch
import torch.nn.functional as F

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def normalize_u8(px, mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD, rescale=1.0 / 255.0):
    """The image processor's rescale + normalise on the host, in float64 rounded to fp32: (x * rescale - mean) / std."""
    m = torch.tensor(mean, dtype=torch.float32).double().view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).double().view(1, -1, 1, 1)
    r = float(torch.tensor(rescale, dtype=torch.float32))
    return ((px.double() * r - m) / s).float()


def clip_vision_forward(sd, pixel_values, heads, act="quick_gelu", eps=1e-5, bf16_storage=False, n_layers=None):
    """sd: state dict with the Hugging Face keys (vision_model.*, visual_projection.weight); pixel_values [B, Cin, S, S] float, already
    normalised.  Returns dict(hidden_states=[L + 1 tensors, index 0 after pre_layrnorm], last_hidden_state (no final norm), pooler_output
    (post_layernorm of the class row), image_embeds)."""
    _st = _round if bf16_storage else (lambda t: t)
    w = (lambda k: _round(sd[k].float())) if bf16_storage else (lambda k: sd[k].float())   # bf16 weight images
    f = lambda k: sd[k].float()                                                              # fp32 biases / affine vectors / class and position embeddings
    v = "vision_model."
    wp = w(v + "embeddings.patch_embedding.weight")
    C, P = wp.shape[0], wp.shape[-1]
    px = _st(pixel_values.float())                                                           # bf16: normalised pixels as patch rows
    B = px.shape[0]
    patch = F.conv2d(px, wp, stride=P).flatten(2).transpose(1, 2)                            # fp32: patch embedding product [B, G, C]
    x = torch.cat([f(v + "embeddings.class_embedding").expand(B, 1, C), patch], 1) + f(v + "embeddings.position_embedding.weight")
    x = _st(F.layer_norm(x, (C,), f(v + "pre_layrnorm.weight"), f(v + "pre_layrnorm.bias"), eps))   # bf16: token rows after pre_layrnorm (hidden_states[0])
    N = x.shape[1]
    d = C // heads
    L = 0
    while v + f"encoder.layers.{L}.layer_norm1.weight" in sd:
        L += 1
    sp = lambda t: t.view(B, N, heads, d).transpose(1, 2)
    hs = [x]
    for i in range(L if n_layers is None else n_layers):
        q = v + f"encoder.layers.{i}."
        h = _st(F.layer_norm(x, (C,), f(q + "layer_norm1.weight"), f(q + "layer_norm1.bias"), eps))            # bf16: LayerNorm1 output
        wqkv = torch.cat([w(q + f"self_attn.{n}_proj.weight") for n in "qkv"], 0)
        bqkv = torch.cat([f(q + f"self_attn.{n}_proj.bias") for n in "qkv"], 0)
        qq, kk, vv = _st(F.linear(h, wqkv, bqkv)).split(C, dim=-1)                                              # bf16: packed q | k | v
        a = (sp(qq) @ sp(kk).transpose(-1, -2)) * d ** -0.5
        o = _st((a.softmax(-1) @ sp(vv)).transpose(1, 2).reshape(B, N, C))                                      # bf16: attention output
        x = _st(x + F.linear(o, w(q + "self_attn.out_proj.weight"), f(q + "self_attn.out_proj.bias")))          # bf16: residual stream after the attention add
        h = _st(F.layer_norm(x, (C,), f(q + "layer_norm2.weight"), f(q + "layer_norm2.bias"), eps))            # bf16: LayerNorm2 output
        u = F.linear(h, w(q + "mlp.fc1.weight"), f(q + "mlp.fc1.bias"))                                         # fp32: fc1 product + bias
        u = _st(u * torch.sigmoid(1.702 * u) if act == "quick_gelu" else F.gelu(u))                             # bf16: activated hidden values
        x = _st(x + F.linear(u, w(q + "mlp.fc2.weight"), f(q + "mlp.fc2.bias")))                                # bf16: residual stream after the MLP add
        hs.append(x)
    pooled = _st(F.layer_norm(hs[-1][:, 0], (C,), f(v + "post_layernorm.weight"), f(v + "post_layernorm.bias"), eps))   # bf16: post_layernorm of the class rows
    embeds = _st(F.linear(pooled, w("visual_projection.weight")))                                               # bf16: image_embeds
    return dict(hidden_states=hs, last_hidden_state=hs[-1], pooler_output=pooled, image_embeds=embeds)


def seeded_state_dict(cfg, seed=0):
    """Seeded weights of a tower of geometry `cfg` (the keys of CLIPVisionModelWithProjection.state_dict()), for sizes no fixture can hold:
    the init transformers gives the vision tower (class embedding N(0, C^-0.5), patch and position embeddings N(0, 0.02); q/k/v std
    C^-0.5 (2L)^-0.5, out_proj C^-0.5, fc1 (2C)^-0.5, fc2 as q/k/v; LayerNorm 1 / 0; projection C^-0.5) with the fixture generator's rescaling
    (matrix weights x 3, biases N(0, 0.1)) so that the logits are not degenerate, every tensor rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    C, I, L, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["patch_size"]
    G = (cfg["image_size"] // P) ** 2
    n = lambda *s, std: torch.randn(*s, generator=g) * std
    in_std, out_std, fc_std = C ** -0.5 * (2 * L) ** -0.5, C ** -0.5, (2 * C) ** -0.5
    v = "vision_model."
    sd = {v + "embeddings.class_embedding": n(C, std=C ** -0.5), v + "embeddings.patch_embedding.weight": n(C, cfg.get("num_channels", 3), P, P, std=0.02),
          v + "embeddings.position_embedding.weight": n(G + 1, C, std=0.02), "visual_projection.weight": n(cfg["projection_dim"], C, std=3.0 * C ** -0.5)}
    for name in ("pre_layrnorm", "post_layernorm"):
        sd[v + name + ".weight"] = torch.ones(C)
        sd[v + name + ".bias"] = n(C, std=0.1)
    for i in range(L):
        q = v + f"encoder.layers.{i}."
        for name, shape, std in (("self_attn.q_proj", (C, C), in_std), ("self_attn.k_proj", (C, C), in_std), ("self_attn.v_proj", (C, C), in_std),
                                 ("self_attn.out_proj", (C, C), out_std), ("mlp.fc1", (I, C), fc_std), ("mlp.fc2", (C, I), in_std)):
            sd[q + name + ".weight"] = n(*shape, std=3.0 * std)
            sd[q + name + ".bias"] = n(shape[0], std=0.1)
        for name in ("layer_norm1", "layer_norm2"):
            sd[q + name + ".weight"] = torch.ones(C)
            sd[q + name + ".bias"] = n(C, std=0.1)
    return {k: _round(t) for k, t in sd.items()}
