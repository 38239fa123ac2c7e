#!/usr/bin/env python3
"""Timing of the Prompt-to-Prompt launches at SD-1.5 geometry (seeded, two prompts: B = 4 = [u_0, u_1, c_0, c_1], 8 heads, 77 keys).

Per cross-attention level (256 / 1024 / 4096 queries, head dim 160 / 80 / 40), on the conditional half (2 samples: the base and one edited):
  fused        one `ops.attention_p2p` launch: both softmaxes, the mapper product, the blend, the product with V and (up to 32 x 32 queries) the store;
  composition  the reference hook's arithmetic in torch on the same bf16 operands: bmm, softmax, einsum with the mapper, the blend, bmm — the
               [2 h, N, 77] logits and probabilities materialised, the store taken as their head sum;
  store only   `ops.attention_p2p` without an output (what AttentionStore adds to a cross-attention call), levels up to 32 x 32 queries;
  core         the plain `ops.attention` on the same two samples, for scale.
  blend        `ops.p2p_local_blend` on five 16 x 16 maps and 2 x 4 x 64 x 64 latents.
Per UNet evaluation (bench.py's SD-1.5 UNet, batch 4, 64 x 64 latents, cached K|V): no controller, AttentionStore, and AttentionReplace with every
gate open (each evaluation is step 0 of a fresh run).

Method: device events around `inner` back-to-back launches, `reps` windows per variant, the variants of a level alternating inside every repetition;
the table gives the median window and the spread (min .. max) per launch in microseconds.  The fused and the composed outputs are compared first.

    python tools/p2p_pair.py [--reps 7] [--inner 50] [--out profiles/p2p_pair.txt] [--no-unet]
"""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from masactrl_pair import alternate  # noqa: E402

BF = torch.bfloat16
LEVELS = ((256, 160), (1024, 80), (4096, 40))
H, P, NK = 8, 2, 77


class _Tok:
    """whole-word tokenizer: enough for word-for-word prompts"""

    def __init__(self):
        self.words = ["<bos>", "<eos>"]

    def encode(self, text):
        ids = [0]
        for w in text.split(" "):
            if w not in self.words:
                self.words.append(w)
            ids.append(self.words.index(w))
        return ids + [1]

    def decode(self, ids):
        return " ".join(self.words[int(i)] for i in ids)


def level_variants(ops, N, D, dev):
    gen = torch.Generator().manual_seed(N + D)
    inner = H * D
    q = torch.randn(P * N, inner, generator=gen).to(BF).to(dev)
    kv = torch.randn(P * NK, 2 * inner, generator=gen).to(BF).to(dev)
    M = torch.zeros(P, NK, NK)
    M[1] = torch.eye(NK)
    M[1, 2, 2], M[1, 2, 3], M[1, 3, 3], M[1, 3, 4] = 0.5, 0.5, 0.0, 1.0          # a replaced word with two target pieces
    c, d = torch.zeros(P, NK), torch.ones(P, NK)
    c[1, :40], d[1, :40] = 1.0, 0.0
    M, c, d = M.to(dev), c.to(dev), d.to(dev)
    scale = D ** -0.5
    qs, ks = (N * inner, D, inner), (NK * 2 * inner, D, 2 * inner)
    stored = N <= 32 ** 2
    out = torch.empty(P, N, inner, dtype=BF, device=dev)
    out_c = torch.empty(P, N, inner, dtype=BF, device=dev)
    store = torch.zeros(P, N, NK, device=dev) if stored else None
    rows = [0, 1] if stored else None

    def fused():
        ops.attention_p2p(q, kv, kv[:, inner:], P, H, N, NK, D, scale, qs, ks, ks, [0, 0], M=M, c=c, d=d, store=store, store_row=rows, out=out)

    def store_only():
        ops.attention_p2p(q, kv, None, P, H, N, NK, D, scale, qs, ks, (0, 0, 0), [0, 1], store=store, store_row=rows, want_out=False)

    def core():
        ops.attention(q, kv, kv[:, inner:], P, H, N, NK, D, scale, qs, ks, ks, out=out_c)

    q4 = q.view(P, N, H, D).permute(0, 2, 1, 3)                                   # [P, H, N, D] views of the same memory
    k4 = kv.view(P, NK, 2, H, D)[:, :, 0].permute(0, 2, 1, 3)
    v4 = kv.view(P, NK, 2, H, D)[:, :, 1].permute(0, 2, 1, 3)
    Mb, cb, db = M[1].to(BF), c[1].to(BF), d[1].to(BF)
    kept = {}

    def composition():
        attn = torch.softmax(torch.matmul(q4, k4.transpose(-1, -2)) * scale, -1)  # [P, H, N, 77] bf16: the reference's attention_probs
        attn[1] = torch.einsum("hpw,wn->hpn", attn[0], Mb) * cb + attn[1] * db
        if stored:
            kept["store"] = attn.float().sum(1)
        out_c.copy_(torch.matmul(attn, v4).permute(0, 2, 1, 3).reshape(P, N, inner))

    fused()
    composition()
    torch.cuda.synchronize()
    diff = float((out.float() - out_c.float()).abs().max() / out_c.float().abs().max())
    variants = {"fused": fused, "composition": composition, "core": core}
    if stored:
        variants["store only"] = store_only
    return variants, diff


def blend_variant(ops, dev):
    gen = torch.Generator().manual_seed(4)
    maps = [torch.rand(2, 256, NK, generator=gen).to(dev) for _ in range(5)]
    x = torch.randn(2, 4, 64, 64, generator=gen).to(dev)
    out = torch.empty_like(x)
    return {"blend": lambda: ops.p2p_local_blend(maps, 16, NK, [[2], [2]], 0.3, x, out=out)}


def unet_variants(dev):
    import bench
    import anyedit_amd.prompt2prompt as PP
    unet, _, _ = bench.build_model(dev)
    model = types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet))
    x_T, img, ehs, null, _, _ = bench.synthetic_inputs(2, dev)
    x = torch.cat([torch.cat([x_T[:1]] * 2), img], 1)
    x = torch.cat([x, x])
    ctx = torch.cat([null.expand(2, -1, -1), ehs])
    t = torch.full((2 * P,), 500, device=dev, dtype=torch.long)
    rows = unet.context_rows(ctx)
    cache = {}
    tok = _Tok()
    prompts = ["a cat sits on the grass", "a dog sits on the grass"]
    ctls = {"no controller": None, "AttentionStore": PP.AttentionStore(),
            "AttentionReplace": PP.AttentionReplace(prompts, 50, 1.0, 1.0, tokenizer=tok)}

    def make(ctl):
        def run():
            PP.unregister(model)
            if ctl is not None:
                ctl.reset()                      # every evaluation is step 0: all gates open, the store overwritten
                PP.register_attention_control(model, ctl)
            unet.forward_rows(x, t, rows, kv_cache=cache)
        return run
    return {k: make(v) for k, v in ctls.items()}, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-unet", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("p2p_pair.py measures on the GPU; none is visible")
    from anyedit_amd import ops
    dev = "cuda"
    lines = [f"Prompt-to-Prompt launches, SD-1.5 geometry, conditional half of B = 4 ({P} samples), {H} heads, {NK} keys; {args.reps} windows of {args.inner} "
             f"launches per variant, alternating; us per call: median (min .. max)", f"device: {torch.cuda.get_device_name(0)}"]
    for N, D in LEVELS:
        variants, diff = level_variants(ops, N, D, dev)
        res = alternate(variants, args.reps, args.inner)
        lines.append(f"N = {N:5d}  d = {D:3d}   fused vs composition output: max |diff| / max = {diff:.2e}")
        for k, (med, lo, hi) in res.items():
            lines.append(f"    {k:12s} {med:9.1f}  ({lo:.1f} .. {hi:.1f})")
        f, c = res["fused"], res["composition"]
        verdict = "fused is faster" if f[2] < c[1] else ("within the spread" if f[1] <= c[2] else "FUSED IS SLOWER than the composition beyond the spread")
        lines.append(f"    fused / composition = {f[0] / c[0]:.3f}   ({verdict})")
    med, lo, hi = alternate(blend_variant(ops, dev), args.reps, args.inner)["blend"]
    lines.append(f"local blend  5 maps 16 x 16 -> 2 x 4 x 64 x 64: {med:9.1f}  ({lo:.1f} .. {hi:.1f})")
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
