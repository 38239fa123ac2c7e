#!/usr/bin/env python3
"""Timing of the MasaCtrl launches at SD-1.5 geometry (seeded, B = 4: [u_s, u_t, c_s, c_t], 8 heads).

Per controlled level (256 / 1024 / 4096 tokens, head dim 160 / 80 / 40):
  fused        one `ops.attention_mutual` launch with classes: all four branches, every target logit computed once, the output written once;
  composition  the same function from the operators the library had before it, without copies: a source launch (`ops.attention` on samples 0 and
               2 through a doubled batch stride), two `key_mask` launches of the target rows on the source's keys (the foreground keys, then the
               complement) and the blend by the target's classes — four launches, the target logits computed twice;
  plain        the stride-only `ops.attention` call of MutualSelfAttentionControl (no classes), for scale;
  token map    `ops.attention_token_map` (256 queries, 77 keys, head dim 160): the launch a 16x16 cross-attention adds under the automatic editor.
Per UNet evaluation (bench.py's SD-1.5 UNet, batch 4, 64 x 64 latents, cached K|V): no editor, MutualSelfAttentionControl,
MutualSelfAttentionControlMask and MutualSelfAttentionControlMaskAuto, each controlling every step from layer 10 on.

Method: device events around `inner` back-to-back launches, `reps` windows per variant, the variants of a level alternating inside every repetition;
the table gives the median window and the spread (min .. max) per launch in microseconds.  The fused and the composed outputs are compared first.

    python tools/masactrl_pair.py [--reps 7] [--inner 50] [--out profiles/masactrl_pair.txt] [--no-unet]
"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
LEVELS = ((256, 160), (1024, 80), (4096, 40))
H, B = 8, 4


def blob(side, cy, cx, r):
    yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
    return (((yy - cy) ** 2 + (xx - cx) ** 2) < r * r).float()


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner   # us per call


def alternate(variants, reps, inner):
    """variants: {name: fn}.  Returns {name: (median, min, max)} us per call."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(window(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def level_variants(ops, N, D, dev):
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(N + D)
    inner = H * D
    ld = 3 * inner
    qkv = torch.randn(B * N, ld, generator=gen).to(BF).to(dev)
    side = int(N ** 0.5)
    ks = F.interpolate(blob(64, 28, 24, 18)[None, None], (side, side)).flatten().to(torch.uint8)
    qt = F.interpolate(blob(64, 36, 40, 16)[None, None], (side, side)).flatten().to(torch.uint8)
    qcls = torch.full((B, N), 255, dtype=torch.uint8)
    qcls[1], qcls[3] = qt, qt
    kcls = ks[None].repeat(B, 1).contiguous()
    ones = int(ks.sum())
    kcnt = torch.tensor([[N - ones, ones]] * B, dtype=torch.int32)
    qcls, kcls, kcnt = qcls.to(dev), kcls.to(dev), kcnt.to(dev)
    scale = D ** -0.5
    s = (N * ld, D, ld)
    s2 = (2 * N * ld, D, ld)                       # every other sample
    k, v = qkv[:, inner:], qkv[:, 2 * inner:]
    out = torch.empty(B, N, inner, dtype=BF, device=dev)
    out_c = torch.empty(B, N, inner, dtype=BF, device=dev)
    o2 = (2 * N * inner, D, inner)
    fg = (ks == 1).to(torch.uint8)[None].repeat(2, 1).contiguous().to(dev)
    bg = (ks == 0).to(torch.uint8)[None].repeat(2, 1).contiguous().to(dev)
    t_fg = torch.empty(2, N, inner, dtype=BF, device=dev)
    t_bg = torch.empty(2, N, inner, dtype=BF, device=dev)
    sel = (qt == 1)[None, :, None].to(dev)
    tq = qkv[N:]                                   # the target samples' rows: 1 and 3 through the doubled stride

    def fused():
        ops.attention_mutual(qkv, k, v, B, H, N, D, scale, s, s, s, (0, 0, 2, 2), qcls=qcls, kcls=kcls, kcnt=kcnt, out=out)

    def composition():
        ops.attention(qkv, k, v, 2, H, N, N, D, scale, s2, s2, s2, out=out_c, o_strides=o2)                      # sources 0, 2 -> out rows 0, 2
        ops.attention(tq, k, v, 2, H, N, N, D, scale, s2, s2, s2, key_mask=fg, out=t_fg)
        ops.attention(tq, k, v, 2, H, N, N, D, scale, s2, s2, s2, key_mask=bg, out=t_bg)
        out_c.view(2, 2, N, inner)[:, 1] = torch.where(sel, t_fg, t_bg)

    def plain():
        ops.attention(qkv, k, v, 2, H, 2 * N, N, D, scale, s2, s2, s2, out=out.view(2, 2 * N, inner))

    fused()
    composition()
    torch.cuda.synchronize()
    diff = float((out.float() - out_c.float()).abs().max() / out_c.float().abs().max())
    return {"fused": fused, "composition": composition, "plain": plain}, diff


def token_map_variant(ops, dev):
    N, Nk, D = 256, 77, 160
    inner = H * D
    gen = torch.Generator().manual_seed(9)
    q = torch.randn(B * N, inner, generator=gen).to(BF).to(dev)
    kv = torch.randn(B * Nk, 2 * inner, generator=gen).to(BF).to(dev)
    out = torch.zeros(B, N, dtype=torch.float32, device=dev)
    sets = [[1]] * 3 + [[1, 2]]

    def token_map():
        ops.attention_token_map(q, kv, B, H, N, Nk, D, D ** -0.5, (N * inner, D, inner), (Nk * 2 * inner, D, 2 * inner), sets, out=out)
    return {"token_map": token_map}


def unet_variants(dev):
    import bench
    import anyedit_amd.masactrl as M
    unet, _, _ = bench.build_model(dev)
    model = types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet))
    x_T, img, ehs, null, _, _ = bench.synthetic_inputs(2, dev)
    x = torch.cat([torch.cat([x_T[:1]] * 2), img], 1)
    x = torch.cat([x, x])
    ctx = torch.cat([null.expand(2, -1, -1), ehs])
    t = torch.full((B,), 500, device=dev, dtype=torch.long)
    rows = unet.context_rows(ctx)
    cache = {}
    kw = dict(start_step=0, start_layer=10, step_idx=range(0, 10 ** 9))   # every evaluation is a controlled step
    editors = {"no editor": None,
               "MutualSelfAttentionControl": M.MutualSelfAttentionControl(**kw),
               "MutualSelfAttentionControlMask": M.MutualSelfAttentionControlMask(**kw, mask_s=blob(64, 28, 24, 18), mask_t=blob(64, 36, 40, 16)),
               "MutualSelfAttentionControlMaskAuto": M.MutualSelfAttentionControlMaskAuto(**kw, thres=0.1, ref_token_idx=[1], cur_token_idx=[1])}

    def make(ed):
        def run():
            if ed is None:
                M.unregister(model)
            elif unet.middle_block[1].transformer_blocks[0].attn1.__dict__.get("editor") is not ed:
                M.register_attention_editor_ldm(model, ed)
            unet.forward_rows(x, t, rows, kv_cache=cache)
        return run
    return {k: make(ed) for k, ed in editors.items()}, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-unet", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masactrl_pair.py measures on the GPU; none is visible")
    from anyedit_amd import ops
    dev = "cuda"
    lines = [f"MasaCtrl launches, SD-1.5 geometry, B = {B}, {H} heads; {args.reps} windows of {args.inner} launches per variant, alternating; us per call: median (min .. max)",
             f"device: {torch.cuda.get_device_name(0)}"]
    for N, D in LEVELS:
        variants, diff = level_variants(ops, N, D, dev)
        res = alternate(variants, args.reps, args.inner)
        lines.append(f"N = {N:5d}  d = {D:3d}   fused vs composition output: max |diff| / max = {diff:.2e}")
        for k, (med, lo, hi) in res.items():
            lines.append(f"    {k:12s} {med:9.1f}  ({lo:.1f} .. {hi:.1f})")
        f, c = res["fused"], res["composition"]
        verdict = "fused is faster" if f[0] < c[0] else ("within the spread" if f[1] <= c[2] else "FUSED IS SLOWER than the composition beyond the spread")
        lines.append(f"    fused / composition = {f[0] / c[0]:.3f}   ({verdict})")
    res = alternate(token_map_variant(ops, dev), args.reps, args.inner)
    med, lo, hi = res["token_map"]
    lines.append(f"token map  N = 256  Nk = 77  d = 160: {med:9.1f}  ({lo:.1f} .. {hi:.1f})")
    if not args.no_unet:
        variants, _ = unet_variants(dev)
        res = alternate(variants, args.reps, 4)
        lines.append("UNet evaluation (batch 4, 64 x 64 latents, cached K|V), ms: median (min .. max)")
        for k, (med, lo, hi) in res.items():
            lines.append(f"    {k:36s} {med / 1e3:8.3f}  ({lo / 1e3:.3f} .. {hi / 1e3:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
