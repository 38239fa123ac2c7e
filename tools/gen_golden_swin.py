"""Fixture generator for GroundingDINO's Swin backbone: tests/golden/swin_tiny_*.npz.

Runs on a development machine only: it loads the reference's own `backbone/swin_transformer.py` BY FILE PATH (pass the reference checkout with
--reference or ANYEDIT_REFERENCE; nothing of it is copied into this tree) behind inert `sys.modules` stubs for the two imports that file makes
and this generator does not need — `timm.models.layers.{DropPath, to_2tuple, trunc_normal_}` (identity, a pair maker, torch's own
trunc_normal_) and `GroundingDINO.groundingdino.util.misc.NestedTensor` (a two-field class) — and runs it on the CPU.  The tests read only the
.npz files.  Chain of trust: the reference's SwinTransformer produces the stored outputs -> tests/swin_ref.py, a plain-torch restatement, is
pinned to them at rel-L2 <= 1e-5 by the CPU suite -> the GPU suite trusts the restatement at sizes no fixture could hold.

Two geometries (patch 4, mlp_ratio 4, head dim 32 at every stage, out_indices over all stages):
  a   window 7,  width 32, depths 2 / 2 / 2, heads 1 / 2 / 4, images 50x38 (patch pad on both axes, a 13x10 grid padded to 14x14, an odd grid into
      PatchMerging, a stage whose map is one window, a stage smaller than the window)
  b   window 12, width 32, depths 2 / 2,     heads 1 / 2,     images 90x106 (a 23x27 grid padded to 24x36: 2x3 windows) and 40x40 (a stage smaller
      than the window)
What the default init leaves degenerate is re-drawn, so that a missing piece shows: relative_position_bias_table from N(0, 0.5^2) (default std
0.02 hides a missing bias), LayerNorm gamma from U(0.25, 1.75) and beta from N(0, 0.1^2) (default 1 / 0), every Linear and conv bias from
N(0, 0.3^2) (default ~0; the qkv bias is what pad tokens attend with).  Every weight is rounded to bf16 BEFORE the reference runs, so the stored
bit patterns are what it computed on.

Files (no file may pass the repository's 1 MiB limit), per geometry <g>:
  swin_tiny_<g>_w<i>.npz           w.<key>: stage i's weights (layers.<i>.*, norm<i>.*; i = 0 also patch_embed.*): floats as bf16 bits (int16), the
                                   persistent relative_position_index buffers as int16
  swin_tiny_<g>_out_<H>x<W>.npz    pixels [2, 3, H, W] fp32; out.<i> = forward_raw(pixels)[i]; stage1_in = the [B, H W, C] input of stage 1 (what
                                   PatchMerging of stage 0 returns); for the first image size of a geometry also mask_in [2, H, W] bool (a
                                   non-trivial padding mask) and mask.<i> = forward(NestedTensor(pixels, mask_in))[i].mask
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOMS = {
    "a": dict(embed_dim=32, depths=[2, 2, 2], num_heads=[1, 2, 4], window_size=7, sizes=[(50, 38)]),
    "b": dict(embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=12, sizes=[(90, 106), (40, 40)]),
}


class NestedTensor:
    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask


def load_reference(root):
    """The reference's swin_transformer module, loaded by path with its two foreign imports stubbed."""
    layers = types.ModuleType("timm.models.layers")
    layers.DropPath = lambda *a, **k: torch.nn.Identity()
    layers.to_2tuple = lambda v: v if isinstance(v, tuple) else (v, v)
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    misc = types.ModuleType("GroundingDINO.groundingdino.util.misc")
    misc.NestedTensor = NestedTensor
    stubs = {"timm": types.ModuleType("timm"), "timm.models": types.ModuleType("timm.models"), "timm.models.layers": layers,
             "GroundingDINO": types.ModuleType("GroundingDINO"), "GroundingDINO.groundingdino": types.ModuleType("GroundingDINO.groundingdino"),
             "GroundingDINO.groundingdino.util": types.ModuleType("GroundingDINO.groundingdino.util"), "GroundingDINO.groundingdino.util.misc": misc}
    for k, v in stubs.items():
        sys.modules.setdefault(k, v)
    path = os.path.join(root, "GroundingDINO", "groundingdino", "models", "GroundingDINO", "backbone", "swin_transformer.py")
    spec = importlib.util.spec_from_file_location("reference_swin_transformer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    ref = load_reference(args.reference)
    import swin_ref
    rel = lambda a, b: float((a.detach().double() - b.detach().double()).norm() / b.detach().double().norm())
    bits = lambda v: v.detach().bfloat16().view(torch.int16).numpy()
    for seed, (name, geom) in enumerate(GEOMS.items()):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(300 + seed)
        kw = {k: v for k, v in geom.items() if k != "sizes"}
        L = len(geom["depths"])
        m = ref.SwinTransformer(pretrain_img_size=224, out_indices=tuple(range(L)), drop_path_rate=0.0, **kw)
        m.eval()                              # the reference's train() override returns None: no chaining
        norms = {k for k, mod in m.named_modules() if isinstance(mod, torch.nn.LayerNorm)}
        with torch.no_grad():
            for k, v in m.named_parameters():
                owner, leaf = k.rsplit(".", 1)
                if leaf == "relative_position_bias_table":
                    v.copy_(torch.randn(v.shape, generator=g) * 0.5)
                elif owner in norms:
                    v.copy_(0.25 + 1.5 * torch.rand(v.shape, generator=g) if leaf == "weight" else torch.randn(v.shape, generator=g) * 0.1)
                elif leaf == "bias":
                    v.copy_(torch.randn(v.shape, generator=g) * 0.3)
                v.copy_(v.bfloat16().float())     # stored as bf16 bit patterns; the reference runs on these values
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for i in range(L):
            own = lambda k: k.startswith((f"layers.{i}.", f"norm{i}.")) or (i == 0 and k.startswith("patch_embed."))
            np.savez_compressed(os.path.join(OUT, f"swin_tiny_{name}_w{i}.npz"),
                                **{"w." + k: (v.numpy().astype(np.int16) if k.endswith("relative_position_index") else bits(v)) for k, v in sd.items() if own(k)})
        grabbed = {}
        m.layers[0].register_forward_hook(lambda mod, inp, out: grabbed.__setitem__("x_down", out[3]))
        for n_size, (H, W) in enumerate(geom["sizes"]):
            px = torch.rand(2, 3, H, W, generator=g)
            with torch.no_grad():
                outs = m.forward_raw(px)
            o = {"pixels": px.numpy(), "stage1_in": grabbed["x_down"].detach().numpy()}
            for i, t in enumerate(outs):
                o[f"out.{i}"] = t.numpy()
            if n_size == 0:
                mask = torch.zeros(2, H, W, dtype=torch.bool)
                mask[0, :, W - W // 2:] = True          # image 0: padded on the right
                mask[1, H - H // 2:, :] = True          # image 1: padded below, and a little on the right
                mask[1, :, W - 5:] = True
                with torch.no_grad():
                    nested = m(NestedTensor(px, mask))
                o["mask_in"] = mask.numpy()
                for i, nt in nested.items():
                    assert torch.equal(nt.tensors, outs[i])
                    o[f"mask.{i}"] = nt.mask.numpy()
            mine = swin_ref.swin_forward(sd, px, kw)
            print(f"{name} {H}x{W}: maps {[tuple(t.shape[1:]) for t in outs]} restatement vs reference rel-L2:",
                  " ".join("%.2e" % rel(a, b) for a, b in zip(mine["outs"], outs)), "stage1_in %.2e" % rel(mine["stage_in"][1], grabbed["x_down"]))
            np.savez_compressed(os.path.join(OUT, f"swin_tiny_{name}_out_{H}x{W}.npz"), **o)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("swin_tiny"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
