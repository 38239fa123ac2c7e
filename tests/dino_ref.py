"""Plain-torch fp32 restatement of the DINOv2 backbone (DinoVisionTransformer: patch convolution with bias, class token, bicubically
interpolated position table, pre-LN blocks with full attention, LayerScale, SwiGLU or GELU FFN, final norm of every row) and of
FrozenDinoV2Encoder's three lines over a state dict — test infrastructure: the CPU suite pins it to tests/golden/dino_tiny_*.npz (which the
reference's own class produced), the GPU suite trusts it at sizes the fixtures cannot hold.

`bf16_storage=True` gives the CONTROL of the project's standing tolerance rule (tests/clip_vision_ref.py's convention): fp32 arithmetic, matrix
weights rounded to bf16 as the module packs them (patch embedding, qkv, w12 / fc1, the projector; `attn.proj` and `mlp.w3` / `mlp.fc2` with their
LayerScale gamma folded in fp32 BEFORE the rounding, their biases gamma * b in fp32) and every activation rounded to bf16 exactly where the
HIP path stores one in HBM.  Each `_st(...)` below is one `# bf16:` mark of anyedit_amd/ldm/modules/encoders/dino_vision.py (run / _normed /
encode_pixels); keep the two lists in step.  NOT rounded: the class token, the position table, the patch bias (fp32 on the HIP path, added
to the fp32 patch product), the patch product, the w12 / fc1 product.
"""
import math

import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def swiglu_hidden(C, mlp_ratio=4.0):
    return (int(int(C * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def pos_table(pos_embed, gh, gw, offset=0.1):
    """interpolate_pos_encoding restated: pos_embed [1, 1 + n n, C] -> [1 + gh gw, C]; rows of the grid scale with gh, columns with gw."""
    pe = pos_embed.float()[0]
    N, C = pe.shape[0] - 1, pe.shape[1]
    if gh * gw == N and gh == gw:
        return pe
    n = int(math.sqrt(N))
    s = math.sqrt(N)
    grid = F.interpolate(pe[1:].reshape(1, n, n, C).permute(0, 3, 1, 2), scale_factor=(float(gh + offset) / s, float(gw + offset) / s), mode="bicubic",
                         antialias=False)
    assert tuple(grid.shape[-2:]) == (gh, gw)
    return torch.cat([pe[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, C)], 0)


def normalize(px, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """FrozenDinoV2Encoder's (image - mean) / std in float64, rounded to fp32."""
    m = torch.tensor(mean, dtype=torch.float32).double().view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).double().view(1, -1, 1, 1)
    return ((px.double() - m) / s).float()


def dino_forward(sd, px, heads, eps=1e-6, offset=0.1, bf16_storage=False, n_blocks=None):
    """sd: state dict with the checkpoint's keys (block_chunks = 0); px [B, Cin, H, W] float, fed to the patch convolution as it is.
    Returns dict(hidden=[x_0 .. x_L], the residual stream in front of block i; normed=[norm(x_i)]; x_prenorm, x_norm_clstoken, x_norm_patchtokens)."""
    _st = _round if bf16_storage else (lambda t: t)
    f = lambda k: sd[k].float()
    w = (lambda k: _round(sd[k].float())) if bf16_storage else f
    wp = w("patch_embed.proj.weight")
    C, P = wp.shape[0], wp.shape[-1]
    x = _st(px.float())                                                                          # bf16: pixels as patch rows
    B, _, H, W = x.shape
    gh, gw = H // P, W // P
    patch = F.conv2d(x, wp, None, stride=P).flatten(2).transpose(1, 2)                           # fp32: patch embedding product [B, G, C]
    patch = patch + f("patch_embed.proj.bias")
    x = torch.cat([f("cls_token").expand(B, 1, C), patch], 1) + pos_table(sd["pos_embed"], gh, gw, offset)
    x = _st(x)                                                                                   # bf16: token rows (no pre-norm)
    N, d = x.shape[1], C // heads
    L = 0
    while f"blocks.{L}.norm1.weight" in sd:
        L += 1
    sp = lambda t: t.view(B, N, heads, d).transpose(1, 2)

    def out_proj(name, q, h, res):
        """res + ls(W h + b): the HIP path folds gamma into W and b; the control rounds the folded matrix."""
        g = f(q + ".gamma") if q + ".gamma" in sd else None
        if not bf16_storage:
            y = F.linear(h, f(name + ".weight"), f(name + ".bias"))
            return res + (y if g is None else g * y)
        wf, bf = f(name + ".weight"), f(name + ".bias")
        if g is not None:
            wf, bf = g[:, None] * wf, g * bf
        return res + F.linear(h, _round(wf), bf)

    hs = [x]
    for i in range(L if n_blocks is None else n_blocks):
        q = f"blocks.{i}."
        h = _st(F.layer_norm(x, (C,), f(q + "norm1.weight"), f(q + "norm1.bias"), eps))                        # bf16: norm1 output
        qq, kk, vv = _st(F.linear(h, w(q + "attn.qkv.weight"), f(q + "attn.qkv.bias"))).split(C, dim=-1)       # bf16: packed q | k | v
        a = (sp(qq) @ sp(kk).transpose(-1, -2)) * d ** -0.5
        o = _st((a.softmax(-1) @ sp(vv)).transpose(1, 2).reshape(B, N, C))                                      # bf16: attention output
        x = _st(out_proj(q + "attn.proj", q + "ls1", o, x))                                                     # bf16: residual stream after the attention add (ls1 folded)
        h = _st(F.layer_norm(x, (C,), f(q + "norm2.weight"), f(q + "norm2.bias"), eps))                        # bf16: norm2 output
        if q + "mlp.w12.weight" in sd:
            u = F.linear(h, w(q + "mlp.w12.weight"), f(q + "mlp.w12.bias"))                                     # fp32: w12 product + bias
            x1, x2 = u.chunk(2, dim=-1)
            u = _st(F.silu(x1) * x2)                                                                            # bf16: gated hidden values
            x = _st(out_proj(q + "mlp.w3", q + "ls2", u, x))                                                    # bf16: residual stream after the FFN add (ls2 folded)
        else:
            u = _st(F.gelu(F.linear(h, w(q + "mlp.fc1.weight"), f(q + "mlp.fc1.bias"))))                        # bf16: activated hidden values
            x = _st(out_proj(q + "mlp.fc2", q + "ls2", u, x))                                                   # bf16: residual stream after the FFN add (ls2 folded)
        hs.append(x)
    normed = [_st(F.layer_norm(h, (C,), f("norm.weight"), f("norm.bias"), eps)) for h in hs]                    # bf16: final norm output
    return dict(hidden=hs, normed=normed, x_prenorm=hs[-1], x_norm_clstoken=normed[-1][:, 0], x_norm_patchtokens=normed[-1][:, 1:])


def intermediate_layers(r, n, gh, gw, reshape=False, return_class_token=False, norm=True):
    """get_intermediate_layers restated over `dino_forward`'s result (block i's output is hidden[i + 1])."""
    L = len(r["hidden"]) - 1
    take = list(range(L - n, L)) if isinstance(n, int) else list(n)
    outs = [(r["normed"] if norm else r["hidden"])[i + 1] for i in take]
    cls = [o[:, 0] for o in outs]
    outs = [o[:, 1:] for o in outs]
    if reshape:
        outs = [o.reshape(o.shape[0], gh, gw, -1).permute(0, 3, 1, 2).contiguous() for o in outs]
    return tuple(zip(outs, cls)) if return_class_token else tuple(outs)


def encoder_forward(sd, image, heads, bf16_storage=False, **kw):
    """FrozenDinoV2Encoder.forward over a `model.*` / `projector.*` state dict: normalise, forward_features, class + patch tokens, projector."""
    tower = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    r = dino_forward(tower, normalize(image), heads, bf16_storage=bf16_storage, **kw)
    wproj = sd["projector.weight"].float()
    hint = F.linear(r["normed"][-1], _round(wproj) if bf16_storage else wproj, sd["projector.bias"].float())
    return _round(hint) if bf16_storage else hint                                                               # bf16: projected hint


def seeded_state_dict(cfg, seed=0, projector_out=None):
    """Seeded weights of a tower of geometry `cfg` (the keys of DinoVisionTransformer.state_dict(); with `projector_out` those of
    FrozenDinoV2Encoder: `model.*` + `projector.*`), for sizes no fixture can hold: the reference's init (Linear weights N(0, 0.02), position
    table N(0, 0.02), patch convolution at its fan-in scale) with the fixture generator's re-draws (matrix weights x 3, biases N(0, 0.1),
    class token N(0, 1), LayerScale gammas U(0.25, 1.75) with a few negative entries), every tensor rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    C, L, P, Cin = cfg["embed_dim"], cfg["depth"], cfg["patch_size"], cfg.get("in_chans", 3)
    G = (cfg["img_size"] // P) ** 2
    swi = cfg["ffn_layer"] in ("swiglufused", "swiglu")
    ratio = cfg.get("mlp_ratio", 4.0)
    Hd = swiglu_hidden(C, ratio) if swi else int(C * ratio)
    n = lambda *s, std: torch.randn(*s, generator=g) * std

    def gamma():
        v = 0.25 + 1.5 * torch.rand(C, generator=g)
        v[::17] *= -1.0
        return v

    sd = {"cls_token": n(1, 1, C, std=1.0), "pos_embed": n(1, G + 1, C, std=0.02), "mask_token": torch.zeros(1, C),
          "patch_embed.proj.weight": n(C, Cin, P, P, std=3.0 * (Cin * P * P) ** -0.5), "patch_embed.proj.bias": n(C, std=0.1),
          "norm.weight": torch.ones(C), "norm.bias": n(C, std=0.1)}
    lin = [("attn.qkv", (3 * C, C)), ("attn.proj", (C, C))] + ([("mlp.w12", (2 * Hd, C)), ("mlp.w3", (C, Hd))] if swi else [("mlp.fc1", (Hd, C)), ("mlp.fc2", (C, Hd))])
    for i in range(L):
        q = f"blocks.{i}."
        for name, shape in lin:
            sd[q + name + ".weight"] = n(*shape, std=3.0 * 0.02)
            sd[q + name + ".bias"] = n(shape[0], std=0.1)
        for name in ("norm1", "norm2"):
            sd[q + name + ".weight"] = torch.ones(C)
            sd[q + name + ".bias"] = n(C, std=0.1)
        if cfg.get("init_values", 1.0):
            sd[q + "ls1.gamma"], sd[q + "ls2.gamma"] = gamma(), gamma()
    if projector_out is not None:
        sd = {"model." + k: v for k, v in sd.items()}
        sd["projector.weight"] = n(projector_out, C, std=3.0 * C ** -0.5)
        sd["projector.bias"] = n(projector_out, std=0.1)
    return {k: _round(t) for k, t in sd.items()}
