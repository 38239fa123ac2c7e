"""Fixture generator for GroundingDINO's neck: tests/golden/gdino_neck.npz.

Runs on a development machine only: it loads the reference's own `models/GroundingDINO/backbone/position_encoding.py` BY FILE PATH (pass the
reference checkout with --reference or ANYEDIT_REFERENCE; nothing of it is copied into this tree) behind an inert `sys.modules` stub for its one
foreign import, `GroundingDINO.groundingdino.util.misc.NestedTensor` (a two-field holder).  The resized masks are torch's own `F.interpolate`,
`get_valid_ratio` is evaluated by the statements of Transformer.get_valid_ratio on those masks, and the two input_proj levels are torch's own
Conv2d + GroupNorm.  The tests read only the .npz file.  Chain of trust: these outputs -> tests/gdino_neck_ref.py, a plain-torch restatement, is
pinned to them by the CPU suite (floats at rel-L2 <= 1e-6, masks and counts exactly) -> the GPU suite trusts the restatement at other sizes.

Stored (all fp32 / bool / int64):
  mask                    [3, 40, 52] image padding masks: sample 0 unpadded, sample 1 padded right and below, sample 2 padded with holes, one fully
                          padded column and one fully padded row
  shapes                  [4, 2] level sizes (10, 13) (5, 7) (3, 4) (2, 2)
  lmask.<l>               F.interpolate(mask[None].float(), size=shapes[l]).to(bool)[0]
  pos.<l>                 PositionEmbeddingSineHW(128, 20, 20, normalize=True)(NestedTensor(x, lmask.<l>))        [3, 256, h, w]
  vr.<l>                  get_valid_ratio(lmask.<l>)                                                              [3, 2]
  proj1.{x,w,b,g,e,y}     Conv2d(48, 256, 1) + GroupNorm(32, 256) on x [2, 48, 5, 7]; weights rounded to bf16 before the reference runs
  proj2.{x,w,b,g,e,y}     Conv2d(48, 256, 3, stride=2, padding=1) + GroupNorm(32, 256) on the same kind of x
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
SHAPES = [(10, 13), (5, 7), (3, 4), (2, 2)]


class _Nested:
    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask


def load_reference(root):
    misc = types.ModuleType("GroundingDINO.groundingdino.util.misc")
    misc.NestedTensor = _Nested
    stubs = {"GroundingDINO": types.ModuleType("GroundingDINO"), "GroundingDINO.groundingdino": types.ModuleType("GroundingDINO.groundingdino"),
             "GroundingDINO.groundingdino.util": types.ModuleType("GroundingDINO.groundingdino.util"), "GroundingDINO.groundingdino.util.misc": misc}
    for k, v in stubs.items():
        sys.modules.setdefault(k, v)
    path = os.path.join(root, "GroundingDINO", "groundingdino", "models", "GroundingDINO", "backbone", "position_encoding.py")
    spec = importlib.util.spec_from_file_location("reference_gdino_position_encoding", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def masks(gen):
    m = torch.zeros(3, 40, 52, dtype=torch.bool)
    m[1, 31:, :] = True
    m[1, :, 37:] = True
    m[2] = torch.rand(40, 52, generator=gen) < 0.3
    m[2, :, 16:20] = True               # level (10, 13) reads column 16 for x = 4: a fully padded column on every level that samples it
    m[2, 24:28, :] = True               # a fully padded row
    return m


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def proj(gen, kernel, stride):
    conv = nn.Conv2d(48, 256, kernel_size=kernel, stride=stride, padding=kernel // 2)
    gn = nn.GroupNorm(32, 256)
    with torch.no_grad():
        a = (3.0 / (48 * kernel * kernel)) ** 0.5
        conv.weight.copy_(bf16_round((torch.rand(conv.weight.shape, generator=gen) * 2 - 1) * a))
        conv.bias.copy_(bf16_round(torch.randn(256, generator=gen) * 0.1))
        gn.weight.copy_(bf16_round(0.5 + torch.rand(256, generator=gen)))
        gn.bias.copy_(bf16_round(torch.randn(256, generator=gen) * 0.1))
        x = bf16_round(torch.randn(2, 48, 5, 7, generator=gen))
        y = gn(conv(x))
    return {"x": x, "w": conv.weight.detach(), "b": conv.bias.detach(), "g": gn.weight.detach(), "e": gn.bias.detach(), "y": y}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"))
    args = ap.parse_args()
    if not args.reference:
        sys.exit("pass --reference <checkout of the reference> (or set ANYEDIT_REFERENCE)")
    ref = load_reference(args.reference)
    gen = torch.Generator().manual_seed(20)
    m = masks(gen)
    out = {"mask": m.numpy(), "shapes": np.asarray(SHAPES, dtype=np.int64)}
    pe = ref.PositionEmbeddingSineHW(128, temperatureH=20, temperatureW=20, normalize=True)
    for l, (h, w) in enumerate(SHAPES):
        lm = F.interpolate(m[None].float(), size=(h, w)).to(torch.bool)[0]
        out[f"lmask.{l}"] = lm.numpy()
        out[f"pos.{l}"] = pe(_Nested(torch.zeros(3, 1, h, w), lm)).numpy()
        valid_H, valid_W = torch.sum(~lm[:, :, 0], 1), torch.sum(~lm[:, 0, :], 1)
        out[f"vr.{l}"] = torch.stack([valid_W.float() / w, valid_H.float() / h], -1).numpy()
    for name, (k, s) in (("proj1", (1, 1)), ("proj2", (3, 2))):
        for key, v in proj(gen, k, s).items():
            out[f"{name}.{key}"] = v.numpy()
    path = os.path.join(OUT, "gdino_neck.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
