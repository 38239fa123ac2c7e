"""Fixture generator for the Prompt-to-Prompt controllers: tests/golden/p2p.npz.

Runs on a development machine only: it imports the reference's own `prompt_to_prompt_stable` module (pass the reference checkout with --reference
or ANYEDIT_REFERENCE; `AnyEdit_Collection/other_modules/prompt2prompt` goes on the path, nothing of it is copied into this tree) and runs its
controller classes on the CPU in fp32.  The module imports diffusers and cv2 at its top and loads a pipeline only to take its tokenizer: stub
modules stand in for both, and the stub pipeline's `from_pretrained` returns an object whose `tokenizer` is the toy tokenizer of
tests/p2p_ref.py.  The tests read only the .npz file.  Chain of trust: the reference's AttentionStore / AttentionReplace / AttentionRefine /
AttentionReweight / LocalBlend / mask_from_CA and its seq_aligner produce the stored arrays -> tests/p2p_ref.py (float64 statements) and the
controller classes of anyedit_amd.prompt2prompt driven on those statements are pinned to them by the CPU suite -> the GPU suite trusts the
statements at the kernels' sizes.

Protocol (constants in tests/p2p_ref.py): the batch [u_0, u_1, c_0, c_1] (one configuration with three prompts), 2 heads of 8 channels, 11
attention calls per step under the place names of G_LAYERS (cross calls at 16 x 16 queries and 77 keys; self calls at 16 x 16 and 17 x 17
tokens), 4 steps with cross_replace_steps = {"default_": 0.5, <word>: (0., 1.)} and self_replace_steps = 0.5.  Every call gets the stored base
operands (bf16 values, stored as their bit patterns) with the queries scaled per call (p2p_ref.call_inputs); attention_probs is formed and handed
to the controller as the reference's registration closure does (ptp_utils.py:219-226), then multiplied with the values.

File (compressed, far below the repository's 1 MiB limit):
  q_all k_all v_all [12, 289, 8], k_cross v_cross [12, 77, 8]   uint16 = bf16 bits, layout (b h) n d, samples [u_0 u_1 u_2 c_0 c_1 c_2]
  latent                fp32 G_LATENT: the latents handed to step_callback, scaled per step (p2p_ref.step_latent)
  out.<config>          fp32 [steps, 11, P, 5, 16]: the conditional half of every call's output at the rows p2p_ref.rows_of(N) (5th row: 289-token calls)
  store.<config>        fp32 [8, P, 4, 77]: the final attention_store of the cross calls, head SUM over the steps, at the rows G_ROWS, in the order
                        down_cross, mid_cross, up_cross
  mapper.* alphas.* alpha.* equalizer.*   the controllers' tables (alpha: cross_replace_alpha [steps + 1, P - 1, 77])
  blend.replace_blend   fp32 [steps, 2, 4, 24, 40]: step_callback's latents; blend_margin: min |normalised map - threshold| over every blend decision
  mask.store            uint8 [256, 256]: mask_from_CA of the store configuration (res 16, from ("up", "down"), G_MASK_WORDS)
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
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    import p2p_ref as R
    tok = R.ToyTokenizer()

    class _Pipe:
        tokenizer = tok

        @classmethod
        def from_pretrained(cls, *a, **k):
            return cls()

        def to(self, *a, **k):
            return self

    df = types.ModuleType("diffusers")
    df.DiffusionPipeline = df.StableDiffusionPipeline = df.StableDiffusionXLPipeline = _Pipe
    sys.modules["diffusers"] = df
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, os.path.join(args.reference, "AnyEdit_Collection", "other_modules", "prompt2prompt"))
    import prompt_to_prompt_stable as P
    P.device = torch.device("cpu")

    gen = torch.Generator().manual_seed(args.seed)
    bh = 6 * R.G_H

    def bf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).bfloat16()

    base = {"q_all": bf(bh, R.G_NMAX, R.G_D, scale=1.5), "k_all": bf(bh, R.G_NMAX, R.G_D, scale=1.5), "v_all": bf(bh, R.G_NMAX, R.G_D),
            "k_cross": bf(bh, R.G_NK, R.G_D, scale=2.0), "v_cross": bf(bh, R.G_NK, R.G_D)}
    g = {k: v.float() for k, v in base.items()}
    g["latent"] = torch.randn(*R.G_LATENT, generator=gen)
    out = {k: v.view(torch.int16).numpy().view(np.uint16) for k, v in base.items()}
    out["latent"] = g["latent"].numpy()
    scale = R.G_D ** -0.5
    margin = float("inf")
    cross_keys = [f"{place}_cross" for place in ("down", "mid", "up")]
    for name, (kind, prompts, word) in R.G_CONFIGS.items():
        ctl = R.make_controller(name, P, None)
        ctl.num_att_layers = len(R.G_LAYERS)
        n = len(prompts)
        outs = torch.zeros(R.G_STEPS, len(R.G_LAYERS), n, len(R.G_ROWS) + 1, R.G_H * R.G_D)
        blends = []
        for step in range(R.G_STEPS):
            for layer in range(len(R.G_LAYERS)):
                place, is_cross, q, k, v = R.call_inputs(g, step, layer, n)
                assert ctl.cur_step == step and ctl.cur_att_layer == layer
                attn = (torch.einsum("b i d, b j d -> b i j", q, k) * scale).softmax(dim=-1)
                attn = ctl(attn, is_cross, place)
                o = torch.bmm(attn, v)                                        # [2 n h, N, d]
                N = o.shape[1]
                o = o.reshape(2 * n, R.G_H, N, R.G_D).permute(0, 2, 1, 3).reshape(2 * n, N, R.G_H * R.G_D)[n:]
                rows = R.rows_of(N)
                outs[step, layer, :, :len(rows)] = o[:, rows]
            if kind == "replace_blend":
                lb = ctl.local_blend
                maps = [m.reshape(2, R.G_H, 256, R.G_NK).sum(1) for m in ctl.attention_store["down_cross"][2:4] + ctl.attention_store["up_cross"][:3]]
                sets = [[int(j) for j in torch.nonzero(lb.alpha_layers[b].flatten()).flatten()] for b in range(2)]
                norm = R.blend_maps(maps, sets, 16, *R.G_LATENT[2:])
                margin = min(margin, float((norm - float(np.float32(lb.threshold))).abs().min()))
                blends.append(ctl.step_callback(R.step_latent(g, step)).clone())
        out["out." + name] = outs.numpy()
        store = [m for key in cross_keys for m in ctl.attention_store[key]]
        out["store." + name] = torch.stack([m.reshape(n, R.G_H, 256, R.G_NK).sum(1)[:, list(R.G_ROWS)] for m in store]).numpy()
        if hasattr(ctl, "cross_replace_alpha"):
            out["alpha." + name] = ctl.cross_replace_alpha.reshape(R.G_STEPS + 1, n - 1, R.G_NK).numpy()
        c0 = getattr(ctl, "prev_controller", None) or ctl
        if hasattr(c0, "mapper"):
            out["mapper." + name] = c0.mapper.numpy()
        if hasattr(c0, "alphas"):
            out["alphas." + name] = c0.alphas.reshape(n - 1, R.G_NK).numpy()
        if hasattr(ctl, "equalizer"):
            out["equalizer." + name] = ctl.equalizer.numpy()
        if blends:
            out["blend." + name] = torch.stack(blends).numpy()
        if kind == "store":
            out["mask.store"] = np.array(P.mask_from_CA(ctl, 16, ("up", "down"), prompts, R.G_MASK_WORDS))
        print(name, "steps", ctl.cur_step, "stored cross maps", len(store))
    if margin < 1e-4:
        raise SystemExit(f"seed {args.seed}: a normalised blend value lies {margin:.2e} from the threshold; pick another seed")
    out["blend_margin"] = np.float64(margin)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "p2p.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, blend margin {margin:.3e}")


if __name__ == "__main__":
    main()
