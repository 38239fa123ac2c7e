"""Fixture generator for the DINOv2 image encoder: tests/golden/dino_tiny_*.npz.

Runs on a development machine only: it imports the reference's own `depth_anything_v2.dinov2` (pass the reference checkout with --reference or
ANYEDIT_REFERENCE; `AnyEdit_Collection/other_modules` goes on the path, nothing of it is copied into this tree) and runs it on the CPU.  The
tests read only the .npz files.  Chain of trust: the reference's DinoVisionTransformer produces the stored outputs -> tests/dino_ref.py, a
plain-torch restatement, is pinned to them at rel-L2 <= 1e-5 by the CPU suite -> the GPU suite trusts the restatement at sizes no fixture
could hold.

Two geometries (depth 2, head dim 64, patch 14, init_values 1.0, interpolate_offset 0.1):
  swiglu   swiglufused, width 128 = 2 x 64, img_size 70 (5 x 5 + 1 positions), mlp_ratio 4 -> hidden 344 (w12 is [688, 128]; 344 is no
           multiple of 64), images 70x70 (native grid), 42x42 (interpolated down), 28x42 (not square)
  mlp      mlp, width 192 = 3 x 64, img_size 56 (4 x 4 + 1 positions), mlp_ratio 2 -> hidden 384, images 56x56, 84x84 (interpolated up)
What the default init leaves degenerate is re-drawn, so that a missing piece shows: ls1 / ls2 gamma from U(0.25, 1.75) with every 17th entry
negative (default: all 1.0), cls_token from N(0, 1) (default std 1e-6), every bias from N(0, 0.1) (default 0), 2-D matrix weights x 3.  Every
weight is rounded to bf16 BEFORE the reference runs, so the stored bit patterns are what it computed on.

Files (no file may pass the repository's 1 MiB limit), per geometry <g>:
  dino_tiny_<g>_w0.npz          w.<key>: the tower's weights except blocks.1 (bf16 bits as int16, the checkpoint's keys, block_chunks = 0);
                                swiglu only: e.projector.weight / e.projector.bias, FrozenDinoV2Encoder's projector (Linear(128, 96))
  dino_tiny_<g>_w1.npz          w.blocks.1.*
  dino_tiny_<g>_out_<H>x<W>.npz pixels [3, 3, H, W] fp32 in [0, 1], image 2 ALL ZERO (visual_reference_tool.py:205); of the reference on
                                `pixels` as they are: x_norm_clstoken, x_norm_patchtokens, x_prenorm, inter.<i>.patch / inter.<i>.cls =
                                get_intermediate_layers(x, n=[0, 1], return_class_token=True, norm=True), pos_interp.<gh>x<gw> =
                                interpolate_pos_encoding for this grid; swiglu only: hint = FrozenDinoV2Encoder.forward(pixels) (its three
                                lines restated here: the reference class opens a checkpoint path when its module is imported)
"""
import argparse
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOMS = {
    "swiglu": dict(embed_dim=128, num_heads=2, depth=2, patch_size=14, img_size=70, mlp_ratio=4.0, ffn_layer="swiglufused", sizes=[(70, 70), (42, 42), (28, 42)]),
    "mlp": dict(embed_dim=192, num_heads=3, depth=2, patch_size=14, img_size=56, mlp_ratio=2.0, ffn_layer="mlp", sizes=[(56, 56), (84, 84)]),
}
PROJECTOR_OUT = 96
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    sys.path.insert(0, os.path.join(args.reference, "AnyEdit_Collection", "other_modules"))
    from depth_anything_v2.dinov2 import DinoVisionTransformer
    from depth_anything_v2.dinov2_layers import MemEffAttention, NestedTensorBlock
    import dino_ref
    rel = lambda a, b: float((a.detach().double() - b.detach().double()).norm() / b.detach().double().norm())
    bits = lambda v: v.detach().bfloat16().view(torch.int16).numpy()
    for seed, (name, geom) in enumerate(GEOMS.items()):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(200 + seed)
        kw = {k: v for k, v in geom.items() if k != "sizes"}
        m = DinoVisionTransformer(init_values=1.0, block_chunks=0, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1,
                                  block_fn=partial(NestedTensorBlock, attn_class=MemEffAttention), **kw).eval()
        projector = torch.nn.Linear(geom["embed_dim"], PROJECTOR_OUT)
        C = geom["embed_dim"]
        with torch.no_grad():
            for k, v in list(m.named_parameters()) + [("projector." + k, v) for k, v in projector.named_parameters()]:
                if v.ndim == 2 and k.endswith("weight"):
                    v.mul_(3.0)
                if k.endswith("bias"):
                    v.copy_(torch.randn(v.shape, generator=g) * 0.1)
                if k.endswith("gamma"):
                    v.copy_(0.25 + 1.5 * torch.rand(v.shape, generator=g))
                    v[::17] *= -1.0
                if k == "cls_token":
                    v.copy_(torch.randn(v.shape, generator=g))
                v.copy_(v.bfloat16().float())     # stored as bf16 bit patterns; the reference runs on these values
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        w0 = {"w." + k: bits(v) for k, v in sd.items() if not k.startswith("blocks.1.")}
        w1 = {"w." + k: bits(v) for k, v in sd.items() if k.startswith("blocks.1.")}
        esd = None
        if name == "swiglu":
            w0.update({"e.projector." + k: bits(v) for k, v in projector.state_dict().items()})
            esd = dict({"model." + k: v for k, v in sd.items()}, **{"projector." + k: v.detach().clone() for k, v in projector.state_dict().items()})
        np.savez_compressed(os.path.join(OUT, f"dino_tiny_{name}_w0.npz"), **w0)
        np.savez_compressed(os.path.join(OUT, f"dino_tiny_{name}_w1.npz"), **w1)
        P = geom["patch_size"]
        for H, W in geom["sizes"]:
            px = torch.rand(3, 3, H, W, generator=g)
            px[2] = 0.0
            gh, gw = H // P, W // P
            with torch.no_grad():
                feats = m.forward_features(px)
                inter = m.get_intermediate_layers(px, n=[0, 1], return_class_token=True, norm=True)
                assert torch.equal(m(px), feats["x_norm_clstoken"])
                pos = m.interpolate_pos_encoding(torch.zeros(1, gh * gw + 1, C), H, W)[0]
            o = {"pixels": px.numpy(), "x_norm_clstoken": feats["x_norm_clstoken"].numpy(), "x_norm_patchtokens": feats["x_norm_patchtokens"].numpy(),
                 "x_prenorm": feats["x_prenorm"].numpy(), f"pos_interp.{gh}x{gw}": pos.detach().numpy()}
            assert feats["x_norm_regtokens"].shape[1] == 0 and feats["masks"] is None
            for i, (patch, cls) in enumerate(inter):
                o[f"inter.{i}.patch"], o[f"inter.{i}.cls"] = patch.numpy(), cls.numpy()
            mine = dino_ref.dino_forward(sd, px, geom["num_heads"])
            line = [f"{name} {H}x{W}: clstoken std {float(feats['x_norm_clstoken'].std()):.3f}", "restatement vs reference rel-L2:",
                    "prenorm %.2e" % rel(mine["x_prenorm"], feats["x_prenorm"]), "patch %.2e" % rel(mine["x_norm_patchtokens"], feats["x_norm_patchtokens"]),
                    "pos %.2e" % rel(dino_ref.pos_table(sd["pos_embed"], gh, gw), pos)]
            if esd is not None:
                with torch.no_grad():   # modules.py:305-311
                    mean, std = (torch.tensor(t).unsqueeze(0).unsqueeze(-1).unsqueeze(-1) for t in (IMAGENET_MEAN, IMAGENET_STD))
                    f = m.forward_features((px - mean) / std)
                    hint = projector(torch.cat([f["x_norm_clstoken"].unsqueeze(1), f["x_norm_patchtokens"]], 1))
                o["hint"] = hint.numpy()
                line.append("hint %.2e" % rel(dino_ref.encoder_forward(esd, px, geom["num_heads"]), hint))
            print(" ".join(line))
            np.savez_compressed(os.path.join(OUT, f"dino_tiny_{name}_out_{H}x{W}.npz"), **o)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("dino_tiny"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
