"""Plain-torch restatement of GroundingDINO's feature enhancer (TransformerEncoder: per layer the image-text fusion BiAttentionBlock, the text
TransformerEncoderLayer and the DeformableTransformerEncoderLayer) over a state dict — test infrastructure: the CPU suite pins it to
tests/golden/gdino_enc_*.npz (which the reference's own classes produced), the GPU suite trusts it at sizes the fixtures cannot hold.

`store=` is the CONTROL of the project's standing tolerance rule: a function applied to every activation exactly where the HIP path stores one in
HBM (`round_bf16` rounds to bf16; None stores nothing).  Each `st(...)` below is one `# bf16:` mark of anyedit_amd/groundingdino/{fuse_modules,
transformer_vanilla,transformer}.py; keep the lists in step.  With a store, matrix weights are rounded to bf16 too, as the module packs them.  NOT
rounded: biases, LayerNorm vectors, gamma_v / gamma_l, the fp32 out-projection products of the fusion, everything inside the deformable attention,
logits and probabilities.

Also here: `bi_attention_float64` and `masked_attention_float64`, the float64 references of the two kernels with the P @ |V| term of the project's
attention rule.
"""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def sine_pos_embed(pos, num_pos_feats, temperature=10000.0, exchange_xy=True):
    """pos [bs, n, k] -> [bs, n, k F]: for coordinate x and feature f, angle = 2 pi x / T^(2 floor(f / 2) / F); even f takes sin, odd f cos."""
    f = torch.arange(num_pos_feats, dtype=torch.float32)
    period = torch.tensor(float(temperature)) ** (2.0 * torch.floor(f / 2.0) / num_pos_feats)
    out = []
    for j in range(pos.shape[-1]):
        ang = pos[..., j, None].float() * (2.0 * math.pi) / period
        out.append(torch.where((torch.arange(num_pos_feats) % 2) == 0, ang.sin(), ang.cos()))
    if exchange_xy:
        out[0], out[1] = out[1], out[0]
    return torch.cat(out, -1)


def reference_points(sizes, valid_ratios):
    """Cell centres of every level, normalised by the valid part of the map, times every level's valid ratio: [bs, sum(HW), L, 2] (x, y)."""
    pts = []
    for lvl, (H, W) in enumerate(sizes):
        y = (torch.arange(H, dtype=torch.float32) + 0.5)[:, None].expand(H, W).reshape(-1)
        x = (torch.arange(W, dtype=torch.float32) + 0.5)[None, :].expand(H, W).reshape(-1)
        ry = y[None] / (valid_ratios[:, None, lvl, 1] * H)
        rx = x[None] / (valid_ratios[:, None, lvl, 0] * W)
        pts.append(torch.stack((rx, ry), -1))
    return torch.cat(pts, 1)[:, :, None] * valid_ratios[:, None]


# ----------------------------------------------------------------------------------------------------------------- float64 kernel references
def bi_attention_float64(q, k, val_v, val_l, heads, scale, mask_v=None, mask_l=None):
    """q / val_v [B, Nv, heads D], k / val_l [B, Nt, heads D]; masks bool, True = padded (removed as a key).  Returns out_v, out_l and the
    P @ |V| terms pav_v, pav_l of the attention rule, all float64 in the inputs' layout."""
    B, Nv, C = q.shape
    Nt = k.shape[1]
    D = C // heads
    sp = lambda t, n: t.double().view(B, n, heads, D).permute(0, 2, 1, 3)
    Q, K, VV, VL = sp(q, Nv), sp(k, Nt), sp(val_v, Nv), sp(val_l, Nt)
    S = scale * Q @ K.transpose(-1, -2)                                   # [B, h, Nv, Nt]
    Sv = S if mask_l is None else S.masked_fill(mask_l.bool()[:, None, None, :], float("-inf"))
    St = S.transpose(-1, -2)
    Sl = St if mask_v is None else St.masked_fill(mask_v.bool()[:, None, None, :], float("-inf"))
    Pv, Pl = Sv.softmax(-1), Sl.softmax(-1)
    un = lambda t, n: t.permute(0, 2, 1, 3).reshape(B, n, C)
    return un(Pv @ VL, Nv), un(Pl @ VV, Nt), un(Pv @ VL.abs(), Nv), un(Pl @ VV.abs(), Nt)


def masked_attention_float64(q, k, v, allowed, heads, scale):
    """q / k / v [B, N, heads D]; allowed bool [B heads, N, N], slice b heads + h, True = the key may be attended.  Returns out, P @ |V|."""
    B, N, C = q.shape
    D = C // heads
    sp = lambda t: t.double().view(B, N, heads, D).permute(0, 2, 1, 3)
    Q, K, V = sp(q), sp(k), sp(v)
    S = (scale * Q @ K.transpose(-1, -2)).masked_fill(~allowed.bool().view(B, heads, N, N), float("-inf"))
    P = S.softmax(-1)
    un = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, C)
    return un(P @ V), un(P @ V.abs())


# ----------------------------------------------------------------------------------------------------------------- the three sub-blocks
class _Ctx:
    def __init__(self, sd, store):
        self.sd, self.store = sd, store

    def st(self, t):
        return t if self.store is None else self.store(t)

    def w(self, key):                      # a matrix weight: rounded as the module packs it when there is a store
        t = self.sd[key].float()
        return t if self.store is None else round_bf16(t)

    def v(self, key):
        return self.sd[key].float()

    def lin(self, x, name):
        return x @ self.w(name + ".weight").t() + self.v(name + ".bias")

    def ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.v(name + ".weight"), self.v(name + ".bias"), LN_EPS)


def _softmax_attend(q, k, v, heads, scale, key_remove=None, allowed=None):
    """fp32 multi-head attention on [B, N, heads D] tensors."""
    B, Nq, C = q.shape
    Nk = k.shape[1]
    D = C // heads
    Q = q.view(B, Nq, heads, D).permute(0, 2, 1, 3)
    K = k.view(B, Nk, heads, D).permute(0, 2, 1, 3)
    V = v.view(B, Nk, heads, D).permute(0, 2, 1, 3)
    S = scale * Q @ K.transpose(-1, -2)
    if key_remove is not None:
        S = S.masked_fill(key_remove.bool()[:, None, None, :], float("-inf"))
    if allowed is not None:
        S = S.masked_fill(~allowed.bool().view(B, heads, Nq, Nk), float("-inf"))
    return (S.softmax(-1) @ V).permute(0, 2, 1, 3).reshape(B, Nq, C)


def fusion_block(c, p, x, t, mask_v, mask_l, heads):
    """BiAttentionBlock: both streams are layer-normed FIRST and the residual is taken from the normed streams."""
    st = c.st
    vn, ln = st(c.ln(x, p + "layer_norm_v")), st(c.ln(t, p + "layer_norm_l"))
    q, vv = st(c.lin(vn, p + "attn.v_proj")), st(c.lin(vn, p + "attn.values_v_proj"))
    k, vl = st(c.lin(ln, p + "attn.l_proj")), st(c.lin(ln, p + "attn.values_l_proj"))
    D = q.shape[-1] // heads
    out_v = st(_softmax_attend(q, k, vl, heads, D ** -0.5, key_remove=mask_l))
    out_l = st(_softmax_attend(k, q, vv, heads, D ** -0.5, key_remove=mask_v))
    x = st(vn + c.v(p + "gamma_v") * c.lin(out_v, p + "attn.out_v_proj"))
    t = st(ln + c.v(p + "gamma_l") * c.lin(out_l, p + "attn.out_l_proj"))
    return x, t


def expand_allowed(allowed, nhead):
    """The reference tiles the batch axis (`repeat(nhead, 1, 1)`) where nn.MultiheadAttention expects slice b nhead + h: that slice therefore
    holds the mask of sample (b nhead + h) mod bs."""
    bs = allowed.shape[0]
    return torch.stack([allowed[(i) % bs] for i in range(bs * nhead)], 0)


def text_layer(c, p, t, pos, allowed_bh, nhead):
    """Post-norm encoder layer: q = k = t + pos, v = t; in_proj rows [0, C) are the query, [C, 2C) the key, [2C, 3C) the value projection."""
    st = c.st
    C = t.shape[-1]
    W, b = c.w(p + "self_attn.in_proj_weight"), c.v(p + "self_attn.in_proj_bias")
    qk_in = st(t + pos) if pos is not None else t
    q = st(qk_in @ W[:C].t() + b[:C])
    k = st(qk_in @ W[C:2 * C].t() + b[C:2 * C])
    v = st(t @ W[2 * C:].t() + b[2 * C:])
    a = st(_softmax_attend(q, k, v, nhead, (C // nhead) ** -0.5, allowed=allowed_bh))
    y = st(t + c.lin(a, p + "self_attn.out_proj"))
    y = st(c.ln(y, p + "norm1"))
    h = st(F.relu(c.lin(y, p + "linear1")))
    z = st(y + c.lin(h, p + "linear2"))
    return st(c.ln(z, p + "norm2"))


def deformable_attention(c, p, query, src, ref_pts, sizes, kpm, heads, points):
    """Multi-scale deformable attention in fp32: per (head, level, point) a bilinear sample (zeros outside, pixel centres at half-integers) of the
    projected values at reference point + offset / (W, H), weighted by a softmax over all levels x points."""
    B, N, C = src.shape
    L, D = len(sizes), C // heads
    lin = lambda x, name: x @ c.v(p + name + ".weight").t() + c.v(p + name + ".bias")      # fp32 on the HIP path: never rounded
    value = lin(src, "value_proj")
    if kpm is not None:
        value = value.masked_fill(kpm.bool()[..., None], 0.0)
    value = value.view(B, N, heads, D)
    off = lin(query, "sampling_offsets").view(B, N, heads, L, points, 2)
    wts = lin(query, "attention_weights").view(B, N, heads, L * points).softmax(-1).view(B, N, heads, L, points)
    wh = torch.tensor([[w, h] for h, w in sizes], dtype=torch.float32)
    loc = ref_pts[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    out = torch.zeros(B, heads, D, N)
    start = 0
    for l, (H, W) in enumerate(sizes):
        img = value[:, start:start + H * W].permute(0, 2, 3, 1).reshape(B * heads, D, H, W)
        grid = (2.0 * loc[:, :, :, l] - 1.0).permute(0, 2, 1, 3, 4).reshape(B * heads, N, points, 2)
        smp = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)          # [B heads, D, N, points]
        wl = wts[:, :, :, l].permute(0, 2, 1, 3).reshape(B * heads, 1, N, points)
        out += (smp * wl).sum(-1).view(B, heads, D, N)
        start += H * W
    out = out.permute(0, 3, 1, 2).reshape(B, N, C)
    return lin(out, "output_proj")


def deform_layer(c, p, x, pos, ref_pts, sizes, kpm, heads, points):
    st = c.st
    d = deformable_attention(c, p + "self_attn.", x + pos if pos is not None else x, x, ref_pts, sizes, kpm, heads, points)
    y = st(x + d)
    y = st(c.ln(y, p + "norm1"))
    h = st(F.relu(c.lin(y, p + "linear1")))
    z = st(y + c.lin(h, p + "linear2"))
    return st(c.ln(z, p + "norm2"))


def encoder_forward(sd, cfg, src, pos, sizes, valid_ratios, key_padding_mask, memory_text, text_attention_mask, pos_text=None,
                    text_self_attention_masks=None, position_ids=None, store=None, tap=None):
    """cfg: num_layers, nhead (deformable heads; text and fusion take nhead // 2), enc_n_points.  sizes: [(H, W)] per level.  Returns
    (output, memory_text) fp32; `tap(layer, name, x, t)` sees both streams after every sub-block."""
    c = _Ctx(sd, store)
    st = c.st
    nl, nhead, points = cfg["num_layers"], cfg["nhead"], cfg.get("enc_n_points", 4)
    bs, n_text, _ = memory_text.shape
    ref_pts = reference_points(sizes, valid_ratios.float())
    if pos_text is None and position_ids is None:
        pos_text = sine_pos_embed(torch.arange(n_text).float()[None, :, None].expand(bs, n_text, 1), 256, exchange_xy=False)
    if position_ids is not None:
        pos_text = sine_pos_embed(position_ids[..., None], 256, exchange_xy=False)
    x, t, pt = st(src.float()), st(memory_text.float()), st(pos_text.float())
    allowed_bh = expand_allowed(text_self_attention_masks.bool(), nhead // 2)
    for i in range(nl):
        x, t = fusion_block(c, f"fusion_layers.{i}.", x, t, key_padding_mask, text_attention_mask, nhead // 2)
        if tap is not None:
            tap(i, "fusion", x, t)
        t = text_layer(c, f"text_layers.{i}.", t, pt, allowed_bh, nhead // 2)
        if tap is not None:
            tap(i, "text", x, t)
        x = deform_layer(c, f"layers.{i}.", x, pos.float(), ref_pts, sizes, key_padding_mask, nhead, points)
        if tap is not None:
            tap(i, "deform", x, t)
    return x, t


def draw_weights(module_state_dict, generator):
    """Seeded weights for a tower no fixture holds, re-drawn as tools/gen_golden_gdino_encoder.py does and rounded to bf16: matrices from
    U(-a, a) with a = sqrt(3 / fan_in) (unit gain), in_proj likewise, gamma_v / gamma_l from U(0.5, 1.5), LayerNorm weights from U(0.5, 1.5) and
    biases from N(0, 0.1^2), every Linear bias from N(0, 0.1^2), the sampling-offset bias kept (it is the reference's ring of directions)."""
    out = {}
    for k, v in module_state_dict.items():
        leaf = k.rsplit(".", 1)[-1]
        r = lambda *s: torch.rand(*s, generator=generator)
        n = lambda *s: torch.randn(*s, generator=generator)
        if leaf in ("gamma_v", "gamma_l"):
            t = 0.5 + r(v.shape)
        elif "norm" in k and leaf == "weight":
            t = 0.5 + r(v.shape)
        elif "norm" in k and leaf == "bias":
            t = 0.1 * n(v.shape)
        elif k.endswith("sampling_offsets.bias"):
            t = v.detach().float().cpu().clone()
        elif k.endswith("sampling_offsets.weight"):
            t = (2 * r(v.shape) - 1) * 0.5 * math.sqrt(3.0 / v.shape[1])
        elif v.dim() == 2:
            t = (2 * r(v.shape) - 1) * math.sqrt(3.0 / v.shape[1])
        else:
            t = 0.1 * n(v.shape)
        out[k] = round_bf16(t.float())
    return out


# ----------------------------------------------------------------------------------------------------------------- fixtures (shared by both test files)
GEOMS = {
    "a": dict(d_model=64, nhead=2, dff=512, num_layers=2, levels=[(9, 7), (5, 4), (3, 2)], wfiles=1),
    "b": dict(d_model=128, nhead=4, dff=1024, num_layers=1, levels=[(12, 10), (6, 5), (3, 3), (2, 2)], wfiles=3),
}


def _golden(name):
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return {k: z[k] for k in z.files}


def _t(a):
    import numpy as np
    return torch.from_numpy(np.asarray(a))


def weights(geom):
    """The stored state dict of a geometry (bf16 bits -> fp32)."""
    sd = {}
    for i in range(GEOMS[geom]["wfiles"]):
        for k, v in _golden(f"gdino_enc_{geom}_w{i}").items():
            assert k.startswith("w.")
            sd[k[2:]] = _t(v).view(torch.bfloat16).float()
    return sd


def stored(geom):
    return _golden(f"gdino_enc_{geom}_io")


def module(geom):
    from anyedit_amd.groundingdino.transformer import build_feature_enhancer
    g = GEOMS[geom]
    return build_feature_enhancer(d_model=g["d_model"], nhead=g["nhead"], dim_feedforward=g["dff"], num_layers=g["num_layers"],
                                  num_feature_levels=len(g["levels"]), enc_n_points=4)


def run_restatement(geom, store=None, tap=None, levels=None):
    """The restatement on a geometry's stored inputs; `levels` runs the same tokens as another level set of equal token count."""
    g, o, sd = GEOMS[geom], stored(geom), weights(geom)
    cfg = dict(num_layers=g["num_layers"], nhead=g["nhead"], enc_n_points=4)
    return encoder_forward(sd, cfg, _t(o["src"]), _t(o["pos"]), levels or g["levels"], _t(o["valid_ratios"]), _t(o["key_padding_mask"]), _t(o["memory_text"]),
                           _t(o["text_attention_mask"]), pos_text=_t(o["pos_text"]), text_self_attention_masks=_t(o["text_self_attention_masks"]),
                           store=store, tap=tap)
