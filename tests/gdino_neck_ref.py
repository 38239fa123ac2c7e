"""Restatement in torch (CPU) of GroundingDINO's neck and grounded-box filter, the reference of tests/test_gdino_neck_cpu.py (which pins it to
tests/golden/gdino_neck.npz, made by the reference's own code) and of tests/test_hip_gdino_neck.py:

    level_mask          F.interpolate(m[None].float(), size=(h, w)).to(bool)[0]  (backbone.py:113, groundingdino.py:306) in integers
    position_sine       PositionEmbeddingSineHW.forward, normalize=True          (position_encoding.py:98-131), any float dtype
    valid_ratio         Transformer.get_valid_ratio
    level_geometry      the three for every level, flattened and concatenated as Transformer.forward does, + level_embed
    input_proj          Conv2d(1x1 | 3x3 stride 2 pad 1) + GroupNorm(32, C)      (groundingdino.py:127-149) on rows
    ground              get_grounding_output's filter                            (tools/tool.py:125-133)
"""
import math

import torch
import torch.nn.functional as F


def level_mask(mask, h, w):
    """mask bool [B, H, W] -> bool [B, h, w]: mask[:, floor(y H / h), floor(x W / w)]"""
    _, H, W = mask.shape
    ys = (torch.arange(h) * H) // h
    xs = (torch.arange(w) * W) // w
    return mask[:, ys][:, :, xs]


def position_sine(mask, num_pos_feats=128, temperatureH=20, temperatureW=20, dtype=torch.float64):
    """mask bool [B, h, w], True = padding -> [B, h, w, 2 * num_pos_feats] (channels last: y half, then x half)"""
    not_mask = ~mask
    y_embed = not_mask.cumsum(1).to(dtype)
    x_embed = not_mask.cumsum(2).to(dtype)
    eps, scale = 1e-6, 2 * math.pi
    y_embed = y_embed / (y_embed[:, -1:, :] + eps) * scale
    x_embed = x_embed / (x_embed[:, :, -1:] + eps) * scale
    i = torch.arange(num_pos_feats, dtype=dtype)
    dim_tx = temperatureW ** (2 * torch.div(i, 2, rounding_mode="floor") / num_pos_feats)
    dim_ty = temperatureH ** (2 * torch.div(i, 2, rounding_mode="floor") / num_pos_feats)
    pos_x = x_embed[..., None] / dim_tx
    pos_y = y_embed[..., None] / dim_ty
    pos_x = torch.stack((pos_x[..., 0::2].sin(), pos_x[..., 1::2].cos()), dim=4).flatten(3)
    pos_y = torch.stack((pos_y[..., 0::2].sin(), pos_y[..., 1::2].cos()), dim=4).flatten(3)
    return torch.cat((pos_y, pos_x), dim=3)


def valid_counts(mask):
    """mask bool [B, h, w] -> integer (unpadded cells of row 0, unpadded cells of column 0), each [B]"""
    return (~mask[:, 0, :]).sum(1), (~mask[:, :, 0]).sum(1)


def valid_ratio(mask):
    _, h, w = mask.shape
    vw, vh = valid_counts(mask)
    return torch.stack([vw.float() / w, vh.float() / h], -1)


def level_geometry(mask, shapes, temperatureH=20, temperatureW=20, level_embed=None, dtype=torch.float64):
    """mask bool [B, H, W] -> (mask_flatten bool [B, N], pos_flatten [B, N, 256] in `dtype` (level_embed added), valid_ratios fp32 [B, L, 2],
    counts: per level the integer (y_embed, x_embed) [B, h, w] pair)"""
    ms, ps, vs, counts = [], [], [], []
    for l, (h, w) in enumerate(shapes):
        m = level_mask(mask, h, w)
        p = position_sine(m, 128, temperatureH, temperatureW, dtype)
        if level_embed is not None:
            p = p + level_embed[l].to(dtype)
        ms.append(m.flatten(1))
        ps.append(p.flatten(1, 2))
        vs.append(valid_ratio(m))
        counts.append(((~m).cumsum(1), (~m).cumsum(2)))
    return torch.cat(ms, 1), torch.cat(ps, 1), torch.stack(vs, 1), counts


def input_proj(x, weight, bias, gamma, beta, stride, groups=32, eps=1e-5):
    """x [B, Cin, H, W]; weight [C, Cin, 1, 1] (stride 1) or [C, Cin, 3, 3] (stride 2, padding 1) -> [B, C, h, w]"""
    y = F.conv2d(x, weight, bias, stride=stride, padding=weight.shape[-1] // 2)
    return F.group_norm(y, groups, gamma, beta, eps)


def ground(pred_logits, pred_boxes, box_threshold, text_threshold):
    """tool.py:125-133 for one image: pred_logits fp32 [nq, T], pred_boxes [nq, 4] -> (kept query indices, scores, boxes, posmaps bool [n, T])"""
    logits = pred_logits.sigmoid()
    score = logits.max(dim=1)[0]
    filt = score > box_threshold
    return torch.nonzero(filt).flatten(), score[filt], pred_boxes[filt], logits[filt] > text_threshold
