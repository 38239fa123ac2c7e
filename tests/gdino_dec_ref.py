"""Plain-torch restatements of the device code of anyedit_amd/csrc/gdino_decoder.hip (GroundingDINO's query selection, decoder bookkeeping and box
head) — test infrastructure: the CPU suite pins them to tests/golden/gdino_dec_geom.npz (which the reference's own functions produced), the GPU
suite trusts them at sizes the fixture does not hold.

`store=` follows tests/gdino_enc_ref.py: a function applied exactly where the HIP path stores bf16 (`round_bf16`; None stores nothing).  The only
bf16 store of these kernels is the sine embedding.
"""
import math

import torch


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def stored(store):
    return (lambda t: t) if store is None else store


def inverse_sigmoid(x, eps=1e-3):
    """log(x / (1 - x)) with x clamped to [0, 1] and both terms of the quotient kept at or above eps."""
    x = x.clamp(0.0, 1.0)
    return torch.log(x.clamp(min=eps) / (1.0 - x).clamp(min=eps))


def encoder_output_proposals(padding_mask, sizes):
    """padding_mask bool [B, N] (True = padding), sizes [(H, W)] -> (proposals fp32 [B, N, 4] un-sigmoided with +inf on padded rows and on rows with
    a coordinate outside (0.01, 0.99), keep bool [B, N]).  A box per cell: centre (x + 0.5, y + 0.5) over the valid extent of the level (counted
    on its first row / first column), side 0.05 * 2^level."""
    B = padding_mask.shape[0]
    rows, start = [], 0
    for lvl, (H, W) in enumerate(sizes):
        m = padding_mask[:, start:start + H * W].view(B, H, W)
        vh = (~m[:, :, 0]).sum(1).to(torch.float32)
        vw = (~m[:, 0, :]).sum(1).to(torch.float32)
        cx = ((torch.arange(W, dtype=torch.float32) + 0.5)[None, None, :] / vw[:, None, None]).expand(B, H, W)
        cy = ((torch.arange(H, dtype=torch.float32) + 0.5)[None, :, None] / vh[:, None, None]).expand(B, H, W)
        side = torch.full((B, H, W), 0.05, dtype=torch.float32) * (2.0 ** lvl)
        rows.append(torch.stack((cx, cy, side, side), -1).reshape(B, H * W, 4))
        start += H * W
    p = torch.cat(rows, 1)
    keep = ((p > 0.01) & (p < 0.99)).all(-1) & ~padding_mask
    logit = torch.log(p / (1.0 - p))
    return torch.where(keep[..., None], logit, torch.full_like(logit, float("inf"))), keep


def reference_points_input(ref, valid_ratios):
    """ref [B, nq, 4], valid_ratios [B, L, 2] -> [B, nq, L, 4]: every box scaled by (rx, ry, rx, ry) of every level."""
    return ref[:, :, None, :] * torch.cat((valid_ratios, valid_ratios), -1)[:, None]


def query_sine_embed(boxes, dtype=torch.float32, store=None):
    """boxes [..., 4] (x, y, w, h) -> [..., 512]: blocks (y, x, w, h) of 128; feature f of a block is sin (f even) / cos (f odd) of
    2 pi c / 10000^(2 floor(f / 2) / 128).  dtype float64 is the kernel test's reference (exact periods)."""
    f = torch.arange(128, dtype=dtype)
    period = torch.tensor(10000.0, dtype=dtype) ** (2.0 * torch.floor(f / 2.0) / 128.0)
    even = (torch.arange(128) % 2) == 0
    out = []
    for c in (1, 0, 2, 3):
        ang = boxes[..., c, None].to(dtype) * (2.0 * math.pi) / period
        out.append(torch.where(even, ang.sin(), ang.cos()))
    return stored(store)(torch.cat(out, -1))


def contrastive(x, y, token_mask, max_text_len):
    """x [B, N, C], y [B, T, C], token_mask bool [B, T] (True = used) -> [B, N, max_text_len], -inf at unused tokens and past T.  Computed in the
    dtype of x."""
    B, N, _ = x.shape
    T = y.shape[1]
    out = torch.full((B, N, max_text_len), float("-inf"), dtype=x.dtype)
    s = x @ y.transpose(1, 2)
    out[..., :T] = torch.where(token_mask[:, None, :], s, torch.full_like(s, float("-inf")))
    return out


def stable_topk(scores, k):
    """The first k indices of a stable descending sort of every row."""
    return torch.sort(scores, dim=1, descending=True, stable=True)[1][:, :k]


def box_refine(h, w3, b3, ref, ref_is_logit=False):
    """(sigmoid(u), u) with u = h w3^T + b3 + (ref if ref_is_logit else inverse_sigmoid(ref))."""
    u = torch.nn.functional.linear(h, w3, b3) + (ref if ref_is_logit else inverse_sigmoid(ref))
    return u.sigmoid(), u


# ----------------------------------------------------------------------------------------------------------------- the tower
# Transformer.forward (flatten, pass-through encoder, two-stage query selection, decoder) and the heads over a state dict.  Each `st(...)` is one
# `# bf16:` mark of anyedit_amd/groundingdino/transformer.py; keep the lists in step.  With a store, the matrix weights that run on ae_gemm_bf16
# are rounded too (enc_output, both attentions' projections, the feed-forward, ref_point_head).  NOT rounded: biases, LayerNorm vectors,
# everything inside the deformable attention, every box MLP, the proposals, logits and probabilities.
import torch.nn.functional as F  # noqa: E402

from gdino_enc_ref import _Ctx, _softmax_attend  # noqa: E402

GEOM = dict(d_model=256, nhead=8, dff=64, num_decoder_layers=2, levels=[(9, 7), (5, 4), (3, 2)], bs=2, num_queries=20, n_text=12, n_text_used_1=7,
            points=4, max_text_len=256)


def _mlp(c, p, x, n):
    """A box MLP, fp32 and never rounded."""
    for i in range(n):
        x = x @ c.v(f"{p}layers.{i}.weight").t() + c.v(f"{p}layers.{i}.bias")
        if i < n - 1:
            x = F.relu(x)
    return x


def deform_cross(c, p, query, mem, rpi, sizes, kpm, heads, points):
    """Deformable cross-attention with reference boxes: query [B, nq, C], mem [B, N, C], rpi [B, nq, L, 4] (cx, cy, w, h per level); a sample sits
    at centre + offset / points * (w, h) / 2."""
    B, N, C = mem.shape
    nq, L, D = query.shape[1], len(sizes), C // heads
    lin = lambda x, name: x @ c.v(p + name + ".weight").t() + c.v(p + name + ".bias")
    value = lin(mem, "value_proj")
    if kpm is not None:
        value = value.masked_fill(kpm.bool()[..., None], 0.0)
    value = value.view(B, N, heads, D)
    off = lin(query, "sampling_offsets").view(B, nq, heads, L, points, 2)
    wts = lin(query, "attention_weights").view(B, nq, heads, L * points).softmax(-1).view(B, nq, heads, L, points)
    box = rpi[:, :, None, :, None, :]
    loc = box[..., :2] + off / points * box[..., 2:] * 0.5
    out = torch.zeros(B, heads, D, nq)
    start = 0
    for l, (H, W) in enumerate(sizes):
        img = value[:, start:start + H * W].permute(0, 2, 3, 1).reshape(B * heads, D, H, W)
        grid = (2.0 * loc[:, :, :, l] - 1.0).permute(0, 2, 1, 3, 4).reshape(B * heads, nq, points, 2)
        smp = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out += (smp * wts[:, :, :, l].permute(0, 2, 1, 3).reshape(B * heads, 1, nq, points)).sum(-1).view(B, heads, D, nq)
        start += H * W
    return lin(out.permute(0, 3, 1, 2).reshape(B, nq, C), "output_proj")


def decoder_layer(c, p, x, qpos, rpi, mem, sizes, kpm, text, text_pad, heads, points, text_cross=True):
    st = c.st
    C = x.shape[-1]
    scale = (C // heads) ** -0.5
    W, b = c.w(p + "self_attn.in_proj_weight"), c.v(p + "self_attn.in_proj_bias")
    qk_in = st(x + qpos)
    q, k = st(qk_in @ W[:C].t() + b[:C]), st(qk_in @ W[C:2 * C].t() + b[C:2 * C])
    v = st(x @ W[2 * C:].t() + b[2 * C:])
    a = st(_softmax_attend(q, k, v, heads, scale))
    y = st(x + c.lin(a, p + "self_attn.out_proj"))
    y = st(c.ln(y, p + "norm2"))
    if text_cross:
        W, b = c.w(p + "ca_text.in_proj_weight"), c.v(p + "ca_text.in_proj_bias")
        q = st(st(y + qpos) @ W[:C].t() + b[:C])
        k, v = st(text @ W[C:2 * C].t() + b[C:2 * C]), st(text @ W[2 * C:].t() + b[2 * C:])
        a = st(_softmax_attend(q, k, v, heads, scale, key_remove=text_pad))
        y = st(y + c.lin(a, p + "ca_text.out_proj"))
        y = st(c.ln(y, p + "catext_norm"))
    d = deform_cross(c, p + "cross_attn.", y + qpos, mem, rpi, sizes, kpm, heads, points)
    y = st(y + d)
    y = st(c.ln(y, p + "norm1"))
    h = st(F.relu(c.lin(y, p + "linear1")))
    z = st(y + c.lin(h, p + "linear2"))
    return st(c.ln(z, p + "norm3"))


def decoder_forward(c, p, cfg, tgt, unsig, mem, sizes, valid_ratios, kpm, text, text_pad, out):
    """TransformerDecoder over tgt [B, nq, C] and un-sigmoided boxes [B, nq, 4]; fills `out` with per-layer taps; returns (hs, references)."""
    st = c.st
    x, ref = st(tgt), unsig.sigmoid()
    hs, refs = [], [ref]
    for l in range(cfg["num_decoder_layers"]):
        rpi = reference_points_input(ref, valid_ratios)
        sine = query_sine_embed(rpi[:, :, 0, :], store=c.store)
        qpos = st(c.lin(st(F.relu(c.lin(sine, p + "ref_point_head.layers.0"))), p + "ref_point_head.layers.1"))
        out[f"dec.{l}.reference_points"], out[f"dec.{l}.query_sine_embed"] = ref, sine
        x = decoder_layer(c, f"{p}layers.{l}.", x, qpos, rpi, mem, sizes, kpm, text, text_pad, cfg["nhead"], cfg["points"], cfg.get("text_cross", True))
        out[f"dec.{l}.output"] = x
        ref = (_mlp(c, f"{p}bbox_embed.{l}.", x, 3) + inverse_sigmoid(ref)).sigmoid()
        refs.append(ref)
        hs.append(st(c.ln(x, p + "norm")))
    return hs, refs


def transformer_forward(sd, cfg, srcs, masks, text, token_mask, two_stage="standard", store=None, topk_proposals=None):
    """srcs [bs, C, h, w] per level, masks bool [bs, h, w] (True = padding), text [bs, T, C], token_mask bool [bs, T] (True = used).  Position
    embeddings do not enter (no encoder layers; the decoder never reads `pos`).  Returns a dict of every tensor the golden stores."""
    c = _Ctx(sd, store)
    st = c.st
    sizes = [tuple(s.shape[-2:]) for s in srcs]
    B = srcs[0].shape[0]
    mem = st(torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1))
    kpm = torch.cat([m.flatten(1) for m in masks], 1)
    vr = torch.stack([torch.stack([(~m[:, 0, :]).sum(1).float() / m.shape[2], (~m[:, :, 0]).sum(1).float() / m.shape[1]], -1) for m in masks], 1)
    textr = st(text)
    out = {}
    nq = cfg["num_queries"]
    if two_stage == "standard":
        prop, keep = encoder_output_proposals(kpm, sizes)
        om = st(c.ln(st(c.lin(mem * keep[..., None], "enc_output")), "enc_output_norm"))
        score = contrastive(om, textr, token_mask, cfg["max_text_len"]).max(-1)[0]
        idx = torch.topk(score, nq, dim=1)[1] if topk_proposals is None else topk_proposals.long()
        out["topk_logits"], out["topk_proposals"] = score, idx
        prop_sel = torch.gather(prop, 1, idx[..., None].expand(-1, -1, 4))
        tgt_undetach = torch.gather(om, 1, idx[..., None].expand(-1, -1, om.shape[-1]))
        unsig = _mlp(c, "enc_out_bbox_embed.", tgt_undetach, 3) + prop_sel
        out["hs_enc"], out["ref_enc"], out["init_box_proposal"] = tgt_undetach[None], unsig.sigmoid()[None], prop_sel.sigmoid()
        tgt = c.v("tgt_embed.weight")[None].expand(B, -1, -1) if cfg.get("embed_init_tgt", True) else tgt_undetach
    else:
        tgt = c.v("tgt_embed.weight")[None].expand(B, -1, -1)
        unsig = c.v("refpoint_embed.weight")[None].expand(B, -1, -1)
        out["init_box_proposal"] = unsig.sigmoid()
    hs, refs = decoder_forward(c, "decoder.", cfg, tgt, unsig, mem, sizes, vr, kpm, textr, ~token_mask, out)
    out["hs"], out["references"] = torch.stack(hs), torch.stack(refs)
    for l, h in enumerate(hs):                                     # groundingdino.py:317-335 on the NORMED outputs
        out[f"pred_boxes.{l}"] = (_mlp(c, f"decoder.bbox_embed.{l}.", h, 3) + inverse_sigmoid(refs[l])).sigmoid()
        out[f"pred_logits.{l}"] = contrastive(h, textr, token_mask, cfg["max_text_len"])
    return out


# ----------------------------------------------------------------------------------------------------------------- fixtures
def _golden_files(prefix):
    import glob
    import os
    import numpy as np
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = {}
    for f in sorted(glob.glob(os.path.join(d, prefix + "*.npz"))):
        with np.load(f) as n:
            z.update({k: n[k] for k in n.files})
    return z


def tower_weights():
    """The golden's state dict (stored as bf16 bits) as fp32 tensors."""
    z = _golden_files("gdino_dec_w")
    return {k[2:]: torch.from_numpy(v).view(torch.bfloat16).float() for k, v in z.items() if k.startswith("w.")}


def tower_io():
    z = _golden_files("gdino_dec_io")
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fbiu" else v) for k, v in z.items()}


def tower_inputs(io):
    L = len(GEOM["levels"])
    return [io[f"src.{l}"] for l in range(L)], [io[f"mask.{l}"] for l in range(L)], [io[f"pos.{l}"] for l in range(L)], io["text"], io["token_mask"]


def tower_module(two_stage="standard", device="cpu"):
    """anyedit_amd's Transformer at the golden's geometry with the heads wired as groundingdino.py:163-197 wires them for the SwinB config (the
    decoder's box head shared, enc_out_bbox_embed a copy of its own), filled from the golden weights through the strict loader."""
    from anyedit_amd.checkpoints import load_groundingdino_transformer
    from anyedit_amd.groundingdino.transformer import Transformer
    from anyedit_amd.groundingdino.utils import MLP, ContrastiveEmbed
    g = GEOM
    m = Transformer(d_model=g["d_model"], nhead=g["nhead"], num_queries=g["num_queries"], num_encoder_layers=0, num_decoder_layers=g["num_decoder_layers"],
                    dim_feedforward=g["dff"], dropout=0.0, return_intermediate_dec=True, num_feature_levels=len(g["levels"]), learnable_tgt_init=True,
                    two_stage_type=two_stage, embed_init_tgt=True, use_text_cross_attention=True)
    box = MLP(256, 256, 4, 3)
    m.decoder.bbox_embed = torch.nn.ModuleList([box] * g["num_decoder_layers"])
    m.decoder.class_embed = torch.nn.ModuleList([ContrastiveEmbed()] * g["num_decoder_layers"])
    sd = tower_weights()
    if two_stage == "standard":
        m.enc_out_bbox_embed, m.enc_out_class_embed = MLP(256, 256, 4, 3), ContrastiveEmbed()
        sd = {k: v for k, v in sd.items() if k != "refpoint_embed.weight"}
    else:
        sd = {k: v for k, v in sd.items() if not k.startswith(("enc_out", "enc_output"))}
    load_groundingdino_transformer(m, sd)
    return m.eval().requires_grad_(False).to(device)
