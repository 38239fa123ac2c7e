"""GroundingDINO/groundingdino/models/GroundingDINO/backbone/backbone.py:146-221 — `Joiner` and `build_backbone` for the Swin towers.

`Joiner(backbone, position_embedding)` is an nn.Sequential as in the reference, so a checkpoint's `backbone.0.*` keys are the tower's and the
position embedding (no parameters) is `backbone.1`.  `forward` is the reference's interface (NCHW maps, a mask and an fp32 embedding per level);
`GroundingDINO.forward` does not go through it: it reads the tower's normed rows (`SwinTransformer.run`) and makes all levels' geometry in one
launch (`ops.gdino_level_geometry`).
"""
import torch.nn as nn

from anyedit_amd.groundingdino.position_encoding import build_position_encoding
from anyedit_amd.groundingdino.swin_transformer import SWIN_GEOMETRIES, build_swin_transformer


class Joiner(nn.Sequential):
    def __init__(self, backbone, position_embedding):
        super().__init__(backbone, position_embedding)
        self.num_channels = None

    def forward(self, tensor_list):
        xs = self[0](tensor_list)
        out, pos = [], []
        for _, x in xs.items():
            out.append(x)
            pos.append(self[1](x).to(x.tensors.dtype))
        return out, pos


def build_backbone(args):
    """:162-221.  Swin only: the ResNet towers are not built on the HIP path."""
    position_embedding = build_position_encoding(args)
    return_interm_indices = list(args.return_interm_indices)
    assert return_interm_indices in [[0, 1, 2, 3], [1, 2, 3], [3]]
    if args.backbone in ("resnet50", "resnet101"):
        raise NotImplementedError(f"build_backbone: the {args.backbone} tower is not built on the HIP path (no FrozenBatchNorm ResNet kernels); the public "
                                  "GroundingDINO checkpoints use swin_T_224_1k and swin_B_384_22k")
    if args.backbone not in SWIN_GEOMETRIES:
        raise NotImplementedError("Unknown backbone {}".format(args.backbone))
    pretrain_img_size = int(args.backbone.split("_")[-2])
    backbone = build_swin_transformer(args.backbone, pretrain_img_size=pretrain_img_size, out_indices=tuple(return_interm_indices), dilation=False,
                                      use_checkpoint=getattr(args, "use_checkpoint", False))
    model = Joiner(backbone, position_embedding)
    model.num_channels = list(backbone.num_features[4 - len(return_interm_indices):])
    return model
