"""Fixture generator for the MasaCtrl editors: tests/golden/masactrl.npz.

Runs on a development machine only: it imports the reference's own `masactrl` package (pass the reference checkout with --reference or
ANYEDIT_REFERENCE; `AnyEdit_Collection/other_modules` goes on the path, nothing of it is copied into this tree) and runs its editor classes
on the CPU in fp32.  The package imports cv2 and torchvision.utils.save_image at its top and uses them only for mask images, which are not
written here: empty stub modules stand in for them (save_image a no-op).  The tests read only the .npz file.  Chain of trust: the
reference's AttentionBase / MutualSelfAttentionControl / MutualSelfAttentionControlMask / MutualSelfAttentionControlMaskAuto produce the
stored outputs -> tests/masactrl_ref.py (float64 statements of the formulas) and the editor classes of anyedit_amd.masactrl driven on those
statements are pinned to them by the CPU suite -> the GPU suite trusts the statements at the kernels' sizes.

Protocol (constants in tests/masactrl_ref.py): the batch [u_s, u_t, c_s, c_t], 2 heads of 8 channels, 16 x 16 queries, 8 text tokens;
6 attention calls per denoising step (three transformer blocks, self then cross), 2 steps, control from step 1 and block 1 on, so that
the calls cross the start step and the start layer.  Every call gets the stored base operands (bf16 values, stored as their bit patterns)
with the queries scaled per call (masactrl_ref.call_inputs); sim and attn are formed as the reference's registration closure forms them
(masactrl_utils.py:176-185).  Configurations: base, plain, mask (two blobs), mask_empty (a source mask without foreground: the reference's
rows of equal logits, i.e. the mean of V), mask_one (a single foreground key), auto (thres 0.5, ref token 1, current tokens 1 and 2).

File (far below the repository's 1 MiB limit):
  q_self k_self v_self [8, 256, 8], q_cross [8, 256, 8], k_cross v_cross [8, 8, 8]   uint16 = bf16 bits, layout (b h) n d
  out.<config>          fp32 [steps, 3 self calls, 4, len(G_ROWS), 16]: the editor's output of every self-attention call at the rows G_ROWS
  controlled.<config>   uint8 [steps, 6]: 1 where the editor's output differs from AttentionBase's (the call was taken over)
  auto_margin           fp64: min |normalised map - thres| over every class decision of `auto` (the generator refuses a seed below 1e-4)
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
    ap.add_argument("--seed", type=int, default=8)
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    sys.path.insert(0, os.path.join(args.reference, "AnyEdit_Collection", "other_modules"))
    sys.modules["cv2"] = types.ModuleType("cv2")
    tv, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")
    tvu.save_image = lambda *a, **k: None
    tv.utils = tvu
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tvu
    from masactrl import masactrl as M
    from masactrl.masactrl_utils import AttentionBase
    import masactrl_ref as R

    gen = torch.Generator().manual_seed(args.seed)
    bh = R.G_B * R.G_H

    def bf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).bfloat16()

    base = {"q_self": bf(bh, R.G_N, R.G_D, scale=1.5), "k_self": bf(bh, R.G_N, R.G_D, scale=1.5), "v_self": bf(bh, R.G_N, R.G_D),
            "q_cross": bf(bh, R.G_N, R.G_D, scale=2.0), "k_cross": bf(bh, R.G_NK, R.G_D, scale=2.0), "v_cross": bf(bh, R.G_NK, R.G_D)}
    g = {k: v.float() for k, v in base.items()}
    scale = R.G_D ** -0.5
    kw = dict(start_step=R.G_START_STEP, start_layer=R.G_START_LAYER, total_steps=R.G_STEPS)

    def editor(name):
        if name == "base":
            return AttentionBase()
        if name == "plain":
            return M.MutualSelfAttentionControl(**kw)
        if name == "auto":
            return M.MutualSelfAttentionControlMaskAuto(**kw, **R.G_AUTO)
        ms, mt = R.golden_masks(name)
        return M.MutualSelfAttentionControlMask(**kw, mask_s=ms, mask_t=mt)

    out = {k: v.view(torch.int16).numpy().view(np.uint16) for k, v in base.items()}
    rows = torch.tensor(R.G_ROWS)
    margin = float("inf")
    for name in R.G_CONFIGS:
        ed = editor(name)
        ed.num_att_layers = R.G_LAYERS
        if name == "auto":   # watch every threshold decision: the normalised map the editor is about to binarise
            agg = ed.aggregate_cross_attn_map

            def watched(idx, agg=agg):
                nonlocal margin
                m = agg(idx)
                margin = min(margin, float((m.double() - R.G_AUTO["thres"]).abs().min()))
                return m
            ed.aggregate_cross_attn_map = watched
        outs = torch.zeros(R.G_STEPS, R.G_LAYERS // 2, R.G_B, len(R.G_ROWS), R.G_H * R.G_D)
        ctl = np.zeros((R.G_STEPS, R.G_LAYERS), dtype=np.uint8)
        for step in range(R.G_STEPS):
            for layer in range(R.G_LAYERS):
                is_cross, q, k, v = R.call_inputs(g, step, layer)
                sim = torch.einsum("b i d, b j d -> b i j", q, k) * scale
                attn = sim.softmax(dim=-1)
                assert ed.cur_step == step and ed.cur_att_layer == layer
                o = ed(q, k, v, sim, attn, is_cross, "input", R.G_H, scale=scale)
                plain = AttentionBase.forward(ed, q, k, v, sim, attn, is_cross, "input", R.G_H)
                ctl[step, layer] = 0 if torch.equal(o, plain) else 1
                if not is_cross:
                    outs[step, layer // 2] = o[:, rows]
        out["out." + name] = outs.numpy()
        out["controlled." + name] = ctl
        print(name, "controlled calls:", ctl.tolist())
    if margin < 1e-4:
        raise SystemExit(f"seed {args.seed}: a normalised map value lies {margin:.2e} from the threshold; pick another seed")
    out["auto_margin"] = np.float64(margin)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "masactrl.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, auto margin {margin:.3e}")


if __name__ == "__main__":
    main()
