"""GroundingDINO/groundingdino/models/GroundingDINO/backbone/position_encoding.py:77-131, :171-186 — the sine position embedding of the image
levels on the HIP path (`ops.gdino_level_geometry`, csrc/gdino_neck.hip).

The detector never calls this module level by level: `GroundingDINO.forward` makes the masks, embeddings and valid ratios of all levels in one
launch, with the temperatures held here.  `forward` exists for callers of the reference's interface and runs the same kernel with one level and
no level embedding; its values are the kernel's (one bf16 rounding) returned in the reference's layout and dtype.
"""
import math

import torch
import torch.nn as nn

from anyedit_amd import ops


class PositionEmbeddingSineHW(nn.Module):
    def __init__(self, num_pos_feats=64, temperatureH=10000, temperatureW=10000, normalize=False, scale=None):
        super().__init__()
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        if scale is None:
            scale = 2 * math.pi
        self.num_pos_feats, self.temperatureH, self.temperatureW, self.normalize, self.scale = num_pos_feats, temperatureH, temperatureW, normalize, scale

    def check_built(self):
        if self.num_pos_feats != 128 or not self.normalize or abs(self.scale - 2 * math.pi) > 1e-12:
            raise NotImplementedError(f"PositionEmbeddingSineHW: built for num_pos_feats=128, normalize=True, scale=2 pi (every GroundingDINO config); got "
                                      f"{self.num_pos_feats}, {self.normalize}, {self.scale}")

    def forward(self, tensor_list):
        """tensor_list: a NestedTensor whose mask is bool [B, h, w] on the GPU -> fp32 [B, 256, h, w]."""
        self.check_built()
        mask = tensor_list.mask
        assert mask is not None
        B, h, w = mask.shape
        _, pos, _ = ops.gdino_level_geometry(mask, [(h, w)], B, self.temperatureH, self.temperatureW)
        return pos.view(B, h, w, 2 * self.num_pos_feats).permute(0, 3, 1, 2).float()


def build_position_encoding(args):
    """:171-186."""
    if args.position_embedding in ("v2", "sine"):
        return PositionEmbeddingSineHW(args.hidden_dim // 2, temperatureH=args.pe_temperatureH, temperatureW=args.pe_temperatureW, normalize=True)
    if args.position_embedding in ("v3", "learned"):
        raise NotImplementedError("build_position_encoding: the learned position embedding is not built: no GroundingDINO config or public checkpoint uses "
                                  "it, and its 50 x 50 table cannot index the 100 x 100 level of an 800-pixel image")
    raise ValueError(f"not supported {args.position_embedding}")
