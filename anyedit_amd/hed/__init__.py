"""HED edge detector on HIP: mirror of AnyEdit_Collection/other_modules/HED/__init__.py (the annotator of the `visual_scribble` condition,
visual_condition_tool.py).  Same class names, parameter names and state-dict keys (`norm`, `blockN.convs.M.{weight,bias}`,
`blockN.projection.{weight,bias}`), so a `ControlNetHED.pth` state dict loads strictly.

Launches of one `detect` at the reference geometry (13 convolutions in 5 blocks):
    stem    ops.hed_stem      x - norm, conv 3 -> 64, bias, ReLU (fp32 weights, direct convolution)
    12 x    ops.conv3x3       the other convolutions, bf16 implicit GEMM with fp32 accumulation, output BEFORE the ReLU
    7 x     ops.relu_         in place, after the convolutions that are not last in their block
    5 x     ops.hed_tail      ReLU + the 1x1 side projection (fp32) + the next block's 2x2 max-pool, the full-resolution ReLU map never written
    1 x     ops.hed_fuse      resize the five side maps, mean, sigmoid, * 255, truncate, invert
Activations between launches are bf16 channels-last rows [B*H*W, C]; the projections and everything after them are fp32.

`nms()` (:77-92) is not built: none of the reference's pipelines calls it.
"""
import types

import numpy as np
import torch
from torch import nn

from anyedit_amd import ops


def _check_side(H, W):
    if H < ops.HED_MIN_SIDE or W < ops.HED_MIN_SIDE:
        raise ValueError(f"HED: a {H} x {W} image is refused: with a side below {ops.HED_MIN_SIDE} pixels the fifth side map would be empty")
    if H > ops.HED_MAX_SIDE or W > ops.HED_MAX_SIDE:
        raise ValueError(f"HED: a {H} x {W} image is refused: sides up to {ops.HED_MAX_SIDE} pixels are covered")


class DoubleConvBlock(nn.Module):
    """:15-31.  Holds the parameters under the reference's names; the arithmetic runs in ControlNetHED_Apache2 (the first convolution of block 1
    is fused with the input normalisation, the last ReLU of every block with its projection and the next block's pooling)."""

    def __init__(self, input_channel, output_channel, layer_number):
        super().__init__()
        self.convs = nn.Sequential()
        self.convs.append(nn.Conv2d(input_channel, output_channel, kernel_size=(3, 3), stride=(1, 1), padding=1))
        for _ in range(1, layer_number):
            self.convs.append(nn.Conv2d(output_channel, output_channel, kernel_size=(3, 3), stride=(1, 1), padding=1))
        self.projection = nn.Conv2d(output_channel, 1, kernel_size=(1, 1), stride=(1, 1), padding=0)

    def packed(self, first):
        """Packed weights of this block, rebuilt when a parameter changes: bf16 implicit-GEMM images of the 3x3 convolutions (block 1's first
        one stays fp32 for the stem kernel), fp32 biases and the fp32 projection."""
        if ops.cache_stale(self, "_pk", *self.parameters()):
            f = lambda t: t.detach().float().contiguous()
            convs = []
            for i, conv in enumerate(self.convs):
                if first and i == 0:
                    convs.append((f(conv.weight), f(conv.bias)))
                else:
                    convs.append((ops.pack_conv3x3(conv.weight.detach().float()), f(conv.bias)))
            self._pk = types.SimpleNamespace(convs=convs, wp=f(self.projection.weight).reshape(-1), bp=f(self.projection.bias).reshape(-1))
        return self._pk


class ControlNetHED_Apache2(nn.Module):
    """:34-51, with the two numbers the reference hard-codes as keywords: `channels` (per block, multiples of 8) and `layers` (convolutions
    per block)."""

    def __init__(self, channels=(64, 128, 256, 512, 512), layers=(2, 2, 3, 3, 3)):
        super().__init__()
        if len(channels) != ops.HED_LEVELS or len(layers) != ops.HED_LEVELS or min(layers) < 1:
            raise ValueError(f"ControlNetHED_Apache2: {ops.HED_LEVELS} blocks of at least one convolution each")
        if any(c % 8 or c < 8 for c in channels) or channels[0] > ops.HED_STEM_CMAX:
            raise ValueError(f"ControlNetHED_Apache2: widths must be multiples of 8 (the first at most {ops.HED_STEM_CMAX}), got {tuple(channels)}")
        self.channels, self.layers = tuple(channels), tuple(layers)
        self.norm = nn.Parameter(torch.zeros(size=(1, 3, 1, 1)))
        cin = 3
        for n, (c, l) in enumerate(zip(channels, layers), 1):
            setattr(self, f"block{n}", DoubleConvBlock(input_channel=cin, output_channel=c, layer_number=l))
            cin = c

    def blocks(self):
        return [getattr(self, f"block{n}") for n in range(1, ops.HED_LEVELS + 1)]

    def _norm(self):
        if ops.cache_stale(self, "_pk", self.norm):
            self._pk = self.norm.detach().float().reshape(-1).contiguous()
        return self._pk

    @torch.no_grad()
    def side_maps(self, x):
        """x: uint8 [B, H, W, 3] or fp32 [B, 3, H, W] on the GPU, channels as the weights expect them.  Returns the five fp32 projections
        [B, H >> k, W >> k]."""
        if x.dim() == 4:
            _check_side(*(x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:4]))
        pk = self.blocks()[0].packed(True)
        h, B, H, W = ops.hed_stem(x, self._norm(), *pk.convs[0])
        sides = []
        for n, blk in enumerate(self.blocks()):
            pk = blk.packed(n == 0)
            last = len(pk.convs) - 1
            for i, (w, b) in enumerate(pk.convs):
                if n or i:
                    h, _, _ = ops.conv3x3(h, w, b, B, H, W)
                    if i < last:
                        ops.relu_(h)
            proj, h = ops.hed_tail(h, pk.wp, pk.bp, B, H, W, pool=n < ops.HED_LEVELS - 1)
            sides.append(proj)
            H, W = H // 2, W // 2
        return sides

    def __call__(self, x):
        """:44-51: x fp32 [B, 3, H, W]; returns the five projections [B, 1, h, w] as fp32."""
        if x.dim() != 4 or x.dtype != torch.float32:
            raise TypeError(f"ControlNetHED_Apache2: expected fp32 [B, 3, H, W], got {x.dtype} {tuple(x.shape)}")
        return tuple(s.unsqueeze(1) for s in self.side_maps(x))


class HEDdetector:
    """:54-74.  `path_or_state_dict`: a `ControlNetHED.pth` file or its state dict (checkpoints.load_hed: strict, `module.` / `netNetwork.`
    prefixes accepted); the geometry keywords are passed on to ControlNetHED_Apache2.

    detect(image_u8)          uint8 [B, H, W, 3] on the GPU -> uint8 edge map [B, H, W] (inverted, as the reference writes it); no host
                              synchronisation, capturable in a graph; `want_logits`: also the fp32 mean logit map the sigmoid is taken of
    detect_array(np_uint8)    [H, W, 3] numpy -> [H, W] numpy
    __call__(image_path, output_path)   the reference's signature
    `detect` and `detect_array` take the channels as given.  The reference reads its file with cv2.imread, which yields BGR, and hands that to a
    network its own header calls RGB-input; `__call__` reproduces that: it flips PIL's RGB to BGR before `detect_array`, and writes the map with PIL
    (cv2 is not a dependency here).

    `nms()` (:77-92) is not built: the reference's pipelines never call it."""

    def __init__(self, path_or_state_dict, device="cuda", **geometry):
        from anyedit_amd.checkpoints import load_hed
        self.netNetwork = ControlNetHED_Apache2(**geometry).float()
        load_hed(self.netNetwork, path_or_state_dict)
        self.netNetwork = self.netNetwork.to(device).eval()

    @torch.no_grad()
    def detect(self, image_u8, invert=True, want_logits=False):
        if image_u8.dim() != 4 or image_u8.dtype != torch.uint8 or image_u8.shape[-1] != 3:
            raise TypeError(f"HEDdetector.detect: expected uint8 [B, H, W, 3], got {image_u8.dtype} {tuple(image_u8.shape)}")
        _check_side(image_u8.shape[1], image_u8.shape[2])
        return ops.hed_fuse(self.netNetwork.side_maps(image_u8), invert=invert, want_logits=want_logits)

    def detect_array(self, image):
        image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
            raise TypeError(f"HEDdetector.detect_array: expected a uint8 [H, W, 3] array, got {image.dtype} {image.shape}")
        _check_side(image.shape[0], image.shape[1])
        dev = self.netNetwork.norm.device
        return self.detect(torch.from_numpy(np.ascontiguousarray(image)).to(dev).unsqueeze(0))[0].cpu().numpy()

    def __call__(self, image_path, output_path):
        from PIL import Image
        rgb = np.array(Image.open(image_path).convert("RGB"))
        edge = self.detect_array(rgb[:, :, ::-1])          # cv2.imread's channel order (:60)
        Image.fromarray(edge).save(output_path)
