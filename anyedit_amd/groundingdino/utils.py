"""GroundingDINO/groundingdino/models/GroundingDINO/utils.py — the three helpers the feature enhancer uses."""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def _get_clones(module, N, layer_share=False):
    """:16-21: N deep copies (or N references when the layers share weights)."""
    if layer_share:
        return nn.ModuleList([module for _ in range(N)])
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def get_sine_pos_embed(pos_tensor, num_pos_feats=128, temperature=10000, exchange_xy=True):
    """:24-53: pos_tensor [bs, n, k] -> [bs, n, k * num_pos_feats]; per coordinate x, feature 2i is sin(2 pi x / T^(2i/F)) and feature 2i + 1 is
    cos(2 pi x / T^(2i/F)), T = temperature, F = num_pos_feats.  exchange_xy swaps the blocks of the first two coordinates."""
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos_tensor.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    blocks = []
    for j in range(pos_tensor.shape[-1]):
        a = pos_tensor[..., j:j + 1] * (2 * math.pi) / dim_t
        blocks.append(torch.stack((a[..., 0::2].sin(), a[..., 1::2].cos()), dim=3).flatten(2))
    if exchange_xy:
        blocks[0], blocks[1] = blocks[1], blocks[0]
    return torch.cat(blocks, dim=-1)


def _get_activation_fn(activation, d_model=256, batch_dim=0):
    """:188-201.  Only relu is built: it is the epilogue of the feed-forward GEMMs (EPI_RELU), and every GroundingDINO config uses it."""
    if activation == "relu":
        return F.relu
    if activation in ("gelu", "glu", "prelu", "selu"):
        raise NotImplementedError(f"activation {activation!r} is not built on the HIP path: the feed-forward GEMMs carry relu only")
    raise RuntimeError(f"activation should be relu/gelu, not {activation}.")
