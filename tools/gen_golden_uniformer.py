"""Fixture generator for the UniFormer backbone: tests/golden/uniformer_tiny_{w,io}.npz.

Runs on a development machine only: it loads the reference's own `other_modules/uniformer/mmseg/models/backbones/uniformer.py` BY FILE PATH (pass
the reference checkout with --reference or ANYEDIT_REFERENCE; nothing of it is copied into this tree) as a member of a made-up package, behind
inert `sys.modules` stubs for its foreign imports: `timm.models.layers` (DropPath = identity, to_2tuple, trunc_normal_), `uniformer.mmcv_custom`
(load_checkpoint, never called: no pretrained path is given), `uniformer.mmseg.utils` (get_root_logger, likewise) and `..builder.BACKBONES` (a
registry whose register_module() returns the class unchanged).  It runs on the CPU.  The tests read only the .npz files.  Chain of trust: the
reference's UniFormer.forward produces the stored maps -> tests/uniformer_ref.py, a plain-torch restatement, is pinned to them at rel-L2 <= 1e-5 by
the CPU suite -> the GPU suite trusts the restatement at the UniFormer-S width, which no fixture could hold.

Geometry: the reference's UniFormer(layers=[1, 1, 2, 1], embed_dim=[16, 32, 64, 64], head_dim=32), windows=False, hybrid=False, .eval().  Weights from
uniformer_ref.seeded_state_dict (BatchNorm running statistics, gamma and beta all non-trivial), loaded strictly.  Images from
uniformer_ref.smooth_pixels: 64x48 (B = 2), 72x56 (maps 18x14, 9x7, 4x3, 2x1: both floors occur) and 40x104.

The fixture condition, asserted here and re-checked by the CPU suite: for every stored level the bf16-storage control's rel-L2 against the reference
lies in [1e-4, 5e-2], so that the GPU suite's `err(HIP) <= 1.5 x err(control)` is neither vacuous nor hopeless.  Seeds are tried in order from
uniformer_ref.TINY_SEED until one meets it; record the seed printed there.

Files (both far below the repository's 1 MiB limit):
  uniformer_tiny_w.npz    w.<key>: the state dict (int16 = bf16 bits for the matrices drawn as bf16 values, float32 / int64 otherwise)
  uniformer_tiny_io.npz   x.<B>x<H>x<W> fp32 [B, 3, H, W], out.<B>x<H>x<W>.<level> fp32 [B, C, h, w] = the reference's four maps
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


def load_reference(root):
    """The reference's backbone module, loaded by path inside a made-up package, its foreign imports stubbed."""
    layers = types.ModuleType("timm.models.layers")
    layers.DropPath = lambda *a, **k: torch.nn.Identity()
    layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    custom = types.ModuleType("uniformer.mmcv_custom")
    custom.load_checkpoint = None
    utils = types.ModuleType("uniformer.mmseg.utils")
    utils.get_root_logger = None
    builder = types.ModuleType("reference_uniformer.builder")
    builder.BACKBONES = types.SimpleNamespace(register_module=lambda: (lambda cls: cls))
    pkg, sub = types.ModuleType("reference_uniformer"), types.ModuleType("reference_uniformer.backbones")
    pkg.__path__, sub.__path__ = [], []
    stubs = {"timm": types.ModuleType("timm"), "timm.models": types.ModuleType("timm.models"), "timm.models.layers": layers,
             "uniformer": types.ModuleType("uniformer"), "uniformer.mmcv_custom": custom, "uniformer.mmseg": types.ModuleType("uniformer.mmseg"),
             "uniformer.mmseg.utils": utils, "reference_uniformer": pkg, "reference_uniformer.builder": builder, "reference_uniformer.backbones": sub}
    for k, v in stubs.items():
        sys.modules.setdefault(k, v)
    path = os.path.join(root, "AnyEdit_Collection", "other_modules", "uniformer", "mmseg", "models", "backbones", "uniformer.py")
    spec = importlib.util.spec_from_file_location("reference_uniformer.backbones.uniformer", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_uniformer.backbones.uniformer"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    ap.add_argument("--seeds", type=int, default=20, help="how many seeds to try from uniformer_ref.TINY_SEED on")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    ref = load_reference(args.reference)
    import uniformer_ref as R
    geo = R.TINY
    net = ref.UniFormer(layers=list(geo["layers"]), embed_dim=list(geo["embed_dim"]), head_dim=geo["head_dim"]).float().eval()
    images = {f"{B}x{H}x{W}": R.smooth_pixels(B, H, W, seed=200 + i) for i, (B, H, W) in enumerate(R.TINY_SIZES)}
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    lo, hi = R.FIXTURE_BAND
    for seed in range(R.TINY_SEED, R.TINY_SEED + args.seeds):
        sd = R.seeded_state_dict(geo["layers"], geo["embed_dim"], geo["head_dim"], seed=seed)
        net.load_state_dict(sd, strict=True)
        io, ok = {}, True
        for name, x in images.items():
            with torch.no_grad():
                outs = net(x)
            mine, ctl = R.forward(sd, x, geo["head_dim"]), R.control(sd, x, geo["head_dim"])
            e_ctl = [rel(c, o) for c, o in zip(ctl, outs)]
            print(f"seed {seed} {name}: maps {[tuple(o.shape[1:]) for o in outs]}; restatement vs reference rel-L2 "
                  + " ".join("%.1e" % rel(m, o) for m, o in zip(mine, outs)) + "; control " + " ".join("%.2e" % e for e in e_ctl)
                  + "; output std " + " ".join("%.2f" % float(o.std()) for o in outs))
            ok &= all(lo <= e <= hi for e in e_ctl)
            io["x." + name] = x.numpy()
            for level, o in enumerate(outs):
                io[f"out.{name}.{level}"] = o.numpy()
        if ok:
            break
        print(f"seed {seed} does not meet the fixture condition")
    assert ok, f"no seed of {args.seeds} met the fixture condition: control rel-L2 in [{lo}, {hi}] at every stored level"
    print(f"seed chosen: {seed} (uniformer_ref.TINY_SEED must name it)")
    assert seed == R.TINY_SEED, "set uniformer_ref.TINY_SEED to the seed chosen and run again"
    w = {}
    for k, v in sd.items():
        if R.stored_as_bf16(k, sd):
            assert torch.equal(v.bfloat16().float(), v), k
            w["w." + k] = v.bfloat16().view(torch.int16).numpy()
        else:
            w["w." + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "uniformer_tiny_w.npz"), **w)
    np.savez_compressed(os.path.join(OUT, "uniformer_tiny_io.npz"), **io)
    for f in ("uniformer_tiny_w.npz", "uniformer_tiny_io.npz"):
        size = os.path.getsize(os.path.join(OUT, f))
        print(f, size)
        assert size < 1 << 20


if __name__ == "__main__":
    main()
