"""Fixture generator for the HED edge detector: tests/golden/hed_tiny_{w,io}.npz.

Runs on a development machine only: it imports the reference's own `HED` module (pass the reference checkout with --reference or
ANYEDIT_REFERENCE; `AnyEdit_Collection/other_modules` goes on the path, nothing of it is copied into this tree) and runs it on the CPU.  The
module imports cv2 at its top and uses it only in HEDdetector and nms(), which are not run here: where cv2 is absent an empty stub module
stands in for it.  The tests read only the .npz files.  Chain of trust: the reference's ControlNetHED_Apache2.__call__ produces the stored
projections -> tests/hed_ref.py, a plain-torch restatement, is pinned to them by the CPU suite -> the GPU suite trusts the restatement at the
full width, which no fixture could hold.

Geometry: the reference's ControlNetHED_Apache2 with its five blocks swapped for narrower instances of the reference's own DoubleConvBlock,
channels (16, 32, 64, 64, 64), layers (2, 2, 3, 3, 3).  Weights from hed_ref.seeded_state_dict (seeded; `norm` = (124, 116, 104); the twelve
wide convolutions' weights are bf16 values and stored as their bit patterns, everything else fp32).  The five projection heads are rescaled
(hed_ref.rescale_heads) so that the mean logit map of the first image has zero mean and standard deviation 2.5: without it the logits reach
+-300 and the edge map is all 0 or 255, which would make every later comparison vacuous.

Files (both far below the repository's 1 MiB limit):
  hed_tiny_w.npz    w.<key>: the state dict (int16 = bf16 bits, float32 otherwise)
  hed_tiny_io.npz   image.<H>x<W> uint8 [H, W, 3] (hed_ref.smooth_image), proj.<H>x<W>.<k> fp32 [1, 1, H >> k, W >> k] = the reference on
                    image.float() as [1, 3, H, W] for sizes 50x38, 64x48, 33x47 (the first and the third are odd at every level)
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    sys.path.insert(0, os.path.join(args.reference, "AnyEdit_Collection", "other_modules"))
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
    from HED import ControlNetHED_Apache2, DoubleConvBlock
    import hed_ref as R
    channels, layers = R.TINY["channels"], R.TINY["layers"]
    net = ControlNetHED_Apache2()
    cin = 3
    for n, (c, l) in enumerate(zip(channels, layers), 1):
        setattr(net, f"block{n}", DoubleConvBlock(input_channel=cin, output_channel=c, layer_number=l))
        cin = c
    net = net.float().eval()
    sd = R.seeded_state_dict(channels, layers, seed=0)
    net.load_state_dict(sd, strict=True)
    images = [R.smooth_image(H, W, seed=100 + i) for i, (H, W) in enumerate(R.TINY_SIZES)]
    H0, W0 = R.TINY_SIZES[0]
    with torch.no_grad():
        raw = net(R.to_nchw(images[0]))
    before = R.mean_logits(list(raw), H0, W0)
    R.rescale_heads(sd, list(raw), H0, W0)
    net.load_state_dict(sd, strict=True)
    print(f"mean logit map of image 0 before the rescale: mean {float(before.mean()):.2f} std {float(before.std()):.2f} "
          f"min {float(before.min()):.1f} max {float(before.max()):.1f}")
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    io = {}
    for img, (H, W) in zip(images, R.TINY_SIZES):
        with torch.no_grad():
            sides = net(R.to_nchw(img))
        io[f"image.{H}x{W}"] = img
        for k, s in enumerate(sides):
            assert tuple(s.shape) == (1, 1, H >> k, W >> k)
            io[f"proj.{H}x{W}.{k}"] = s.numpy()
        m = R.mean_logits(list(sides), H, W)
        e = R.edge_map(list(sides), H, W)
        mine = R.forward(sd, R.to_nchw(img))
        ctl = R.control(sd, R.to_nchw(img))
        print(f"{H}x{W}: mean logit mean {float(m.mean()):+.3f} std {float(m.std()):.3f}; edge map pixels strictly between 5 and 250: "
              f"{100.0 * float(((e > 5) & (e < 250)).float().mean()):.1f} %; restatement vs reference rel-L2 "
              + " ".join("%.1e" % rel(a, b) for a, b in zip(mine, sides))
              + f"; control mean-logit rel-L2 {rel(R.mean_logits(ctl, H, W), m):.2e}")
    bits = lambda v: v.detach().bfloat16().view(torch.int16).numpy()
    w = {}
    for k, v in sd.items():
        wide = k.endswith("weight") and ".convs." in k and not k.startswith("block1.convs.0.")
        if wide:
            assert torch.equal(v.bfloat16().float(), v), k
        w["w." + k] = bits(v) if wide else v.numpy()
    np.savez_compressed(os.path.join(OUT, "hed_tiny_w.npz"), **w)
    np.savez_compressed(os.path.join(OUT, "hed_tiny_io.npz"), **io)
    for f in ("hed_tiny_w.npz", "hed_tiny_io.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
