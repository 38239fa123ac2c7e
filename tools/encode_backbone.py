"""Time of one forward of GroundingDINO's image backbone (groundingdino/swin_transformer.py: what the detector of tools/tool.py:91-102 runs on
its 800-pixel image), Swin-B-384 geometry (width 128, depths 2 / 2 / 18 / 2, heads 4 / 8 / 16 / 32, window 12), seeded weights, one 800x800 image:
eager (launch-per-op from Python) and as a replayed graph — and next to it the yardstick: the same backbone run by torch's own bf16 operators on
the same GPU in the same process (tests/swin_ref.py's statements on bf16 tensors: F.conv2d, F.layer_norm, pad / roll / partition, F.linear,
F.scaled_dot_product_attention with the additive bias + shift mask on the partitioned windows, reverse / roll / crop, F.gelu), eager and
replayed — and the time of the new attention launch alone at every stage's shape, un-shifted and shifted.

    python tools/encode_backbone.py [--iters 10] [--warmup 3] [--size 800] [--depths 2 2 18 2] [--step-timeout 400] [--out FILE]

The measurement runs in a child process under `--step-timeout` seconds (this process never opens the GPU).  Each figure is a host clock around
`iters` forwards that ends in a device synchronise (the clock is read after the synchronise), after `warmup` untimed forwards of the same
shape; the window is repeated 3 times and the median is reported with the spread.  Prints one JSON line.  These are reports, not gates.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters, warmup, windows=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / iters)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def torch_bf16_backbone(sd, cfg):
    """The backbone on torch's bf16 operators: weights and activations bf16 on the GPU; the additive attention masks (bias, and bias + shift mask
    per window) are made once per map size, outside the timed region."""
    import torch
    import torch.nn.functional as F
    import swin_ref as R
    w = {k: (v.to("cuda", torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()}
    ws, depths, heads = cfg["window_size"], cfg["depths"], cfg["num_heads"]
    masks = {}

    def mask_of(key, i, j, Hp, Wp, shift):
        k = (i, j, Hp, Wp)
        if k not in masks:
            b = R.gathered_bias(sd[key].float(), ws)                                                # [nH, N, N]
            m = b[None] if shift == 0 else b[None] + R.shift_mask(Hp, Wp, ws, shift)[:, None]        # [1 | nW, nH, N, N]
            masks[k] = m.to("cuda", torch.bfloat16)
        return masks[k]

    def run(px):
        x = px.to(torch.bfloat16)
        B, _, H, W = x.shape
        x = F.pad(x, (0, R.up(W, 4) - W, 0, R.up(H, 4) - H))
        x = F.conv2d(x, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], stride=4)
        H, W = x.shape[2:]
        x = x.flatten(2).transpose(1, 2)
        x = F.layer_norm(x, x.shape[-1:], w["patch_embed.norm.weight"], w["patch_embed.norm.bias"], 1e-5)
        outs = []
        for i, depth in enumerate(depths):
            C, nH, N = x.shape[-1], heads[i], ws * ws
            Hp, Wp = R.up(H, ws), R.up(W, ws)
            nW = (Hp // ws) * (Wp // ws)
            for j in range(depth):
                q = f"layers.{i}.blocks.{j}."
                shift = 0 if j % 2 == 0 else ws // 2
                h = F.layer_norm(x, (C,), w[q + "norm1.weight"], w[q + "norm1.bias"], 1e-5)
                h = F.pad(h.view(B, H, W, C), (0, 0, 0, Wp - W, 0, Hp - H))
                if shift:
                    h = torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
                win = F.linear(R.partition(h, ws), w[q + "attn.qkv.weight"], w[q + "attn.qkv.bias"]).view(-1, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
                m = mask_of(q + "attn.relative_position_bias_table", i, j, Hp, Wp, shift)
                if shift:
                    o = F.scaled_dot_product_attention(win[0].view(B, nW, nH, N, 32), win[1].view(B, nW, nH, N, 32), win[2].view(B, nW, nH, N, 32), attn_mask=m[None])
                    o = o.view(B * nW, nH, N, 32)
                else:
                    o = F.scaled_dot_product_attention(win[0], win[1], win[2], attn_mask=m)
                o = F.linear(o.transpose(1, 2).reshape(-1, N, C), w[q + "attn.proj.weight"], w[q + "attn.proj.bias"])
                o = R.reverse(o, ws, Hp, Wp)
                if shift:
                    o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
                x = x + o[:, :H, :W].reshape(B, H * W, C)
                h = F.layer_norm(x, (C,), w[q + "norm2.weight"], w[q + "norm2.bias"], 1e-5)
                x = x + F.linear(F.gelu(F.linear(h, w[q + "mlp.fc1.weight"], w[q + "mlp.fc1.bias"])), w[q + "mlp.fc2.weight"], w[q + "mlp.fc2.bias"])
            z = F.layer_norm(x, (C,), w[f"norm{i}.weight"], w[f"norm{i}.bias"], 1e-5)
            outs.append(z.view(B, H, W, C).permute(0, 3, 1, 2).contiguous())
            d = f"layers.{i}.downsample."
            if d + "reduction.weight" in w:
                x = F.linear(F.layer_norm(R.merge_rows(x, H, W), (4 * C,), w[d + "norm.weight"], w[d + "norm.bias"], 1e-5), w[d + "reduction.weight"])
                H, W = (H + 1) // 2, (W + 1) // 2
        return tuple(outs)

    return run


def measure(size, depths, iters, warmup):
    import torch
    import swin_ref as R
    from anyedit_amd import _lib, ops
    from anyedit_amd.groundingdino.swin_transformer import build_swin_transformer
    cfg = dict(R.GEOMETRIES["swin_B_384_22k"], depths=depths)
    sd = R.seeded_state_dict(cfg, seed=0)
    with torch.device("meta"):
        m = build_swin_transformer("swin_B_384_22k", 384, depths=depths)
    m.load_state_dict(sd, assign=True)
    m = m.to("cuda").eval()
    px = torch.rand(1, 3, size, size, generator=torch.Generator().manual_seed(1)).to("cuda")
    ref = torch_bf16_backbone(sd, cfg)
    r = lambda v: round(v, 4)
    with torch.no_grad():
        eager = timed(lambda: m.forward_raw(px), iters, warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = m.forward_raw(px)
        replay = timed(graph.replay, iters, warmup)
        t_eager = timed(lambda: ref(px), iters, warmup)
        tgraph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(tgraph):
            touts = ref(px)
        t_replay = timed(tgraph.replay, iters, warmup)
        torch.cuda.synchronize()
        agree = []
        for a, b in zip(outs, touts):
            assert torch.isfinite(a).all() and torch.isfinite(b.float()).all()
            agree.append(r(float((a.float() - b.float()).norm() / b.float().norm())))
        # the new attention launch alone, at every stage's shape: the stage's own buffers and packed bias, 4 x iters launches per window
        ws = m.run(px)
        attn = []
        for st, layer in zip(ws.stages, m.layers):
            p = layer.blocks[1].packed()
            for shift in (0, m.window_size // 2):
                t = timed(lambda: ops.swin_window_attention(st.qkv, p.bqkv, p.rpb, 1, st.H, st.W, layer.num_heads, m.window_size, shift, 32 ** -0.5, out=st.att),
                          4 * iters, warmup)
                nW = -(-st.H // m.window_size) * -(-st.W // m.window_size)
                attn.append({"map": [st.H, st.W], "heads": layer.num_heads, "windows": nW, "shift": shift, "blocks_in_stage": len(layer.blocks),
                             "ms": r(t[0]), "min_max_ms": [r(t[1]), r(t[2])]})
    per_forward = sum(a["ms"] * a["blocks_in_stage"] / 2 for a in attn)
    return {"device": _lib.device_arch(), "geometry": f"Swin-B-384 (width 128, window 12), depths {depths}, one {size}x{size} image", "iters": iters, "warmup": warmup,
            "eager_ms": r(eager[0]), "eager_min_max_ms": [r(eager[1]), r(eager[2])], "graph_replay_ms": r(replay[0]), "graph_min_max_ms": [r(replay[1]), r(replay[2])],
            "torch_bf16_eager_ms": r(t_eager[0]), "torch_bf16_eager_min_max_ms": [r(t_eager[1]), r(t_eager[2])],
            "torch_bf16_graph_replay_ms": r(t_replay[0]), "torch_bf16_graph_min_max_ms": [r(t_replay[1]), r(t_replay[2])],
            "hip_over_torch_graph": r(replay[0] / t_replay[0]), "hip_over_torch_eager": r(eager[0] / t_eager[0]), "rel_l2_hip_vs_torch_bf16_per_map": agree,
            "window_attention_launch": attn, "window_attention_ms_per_forward": r(per_forward)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--depths", type=int, nargs=4, default=[2, 2, 18, 2])
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", action="store_true", help="(internal) measure in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.size, a.depths, a.iters, a.warmup)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", "--iters", str(a.iters), "--warmup", str(a.warmup),
           "--size", str(a.size), "--depths"] + [str(d) for d in a.depths]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if res.returncode != 0:
        print(f"the measuring process ended with status {res.returncode}", file=sys.stderr)
        return res.returncode
    line = res.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
