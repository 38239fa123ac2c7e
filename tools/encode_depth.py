"""Time of one depth map (depth_anything_v2.DepthAnythingV2: what the `visual_depth` condition costs per image), reference geometry (ViT-L tower,
head features 256 on levels of 256 / 512 / 1024 / 1024 channels), seeded weights with the last layer rescaled on the image, one 518x518 image:
`forward` (tower + head, fp32 depth) and `detect` (+ normalisation in the patch launch, the resize to the image's size with its min / max, the colour
image), eager (launch-per-op from Python) and as a replayed graph, next to the same network on torch's own bf16 operators (F.linear /
scaled_dot_product_attention / layer_norm for the tower, channels-last F.conv2d / conv_transpose2d / interpolate for the head), and the per-launch
table of one eager detect (HIP events around every launch).

    python tools/encode_depth.py [--iters 20] [--warmup 5] [--size 518] [--step-timeout 420] [--out FILE]

The measurement runs in a child process of its own under `--step-timeout` seconds (this process never opens the GPU); if it fails or runs out of
time nothing else is started.  Each figure is a host clock around `iters` calls that ends in a device synchronise, after `warmup` untimed calls; the
window is repeated 3 times and the median is reported with the spread.  Arithmetic at 518x518 (a 37 x 37 grid): the tower about 1 TFLOP, the head
about 220 GFLOP.
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
    return [round(v, 4) for v in (ms[len(ms) // 2], ms[0], ms[-1])]


def torch_bf16_forward(sd, heads, layers):
    """The same network on torch's operators: bf16 weights and activations, fp32 accumulation inside the operators, fp32 depth."""
    import torch
    import torch.nn.functional as F
    import dino_ref
    import dpt_ref as R
    bf = torch.bfloat16
    tower, head = R.split(sd)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
    tw = {k: v.to("cuda", bf) for k, v in tower.items()}
    hd = {k: cl(v.to("cuda", bf)) for k, v in head.items()}
    C = tw["cls_token"].shape[-1]
    L = max(layers) + 1
    pos = {}

    def run(x):
        B, _, H, W = x.shape
        gh, gw = H // 14, W // 14
        if (gh, gw) not in pos:
            pos[(gh, gw)] = dino_ref.pos_table(tower["pos_embed"], gh, gw).to("cuda", bf)
        t = F.conv2d(x.to(bf), tw["patch_embed.proj.weight"], tw["patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)
        t = torch.cat([tw["cls_token"].expand(B, 1, C), t], 1) + pos[(gh, gw)]
        N, d = t.shape[1], C // heads
        feats = []
        for i in range(L):
            q = f"blocks.{i}."
            h = F.layer_norm(t, (C,), tw[q + "norm1.weight"], tw[q + "norm1.bias"], 1e-6)
            qkv = F.linear(h, tw[q + "attn.qkv.weight"], tw[q + "attn.qkv.bias"]).view(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
            o = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B, N, C)
            t = t + tw[q + "ls1.gamma"] * F.linear(o, tw[q + "attn.proj.weight"], tw[q + "attn.proj.bias"])
            h = F.layer_norm(t, (C,), tw[q + "norm2.weight"], tw[q + "norm2.bias"], 1e-6)
            h = F.linear(F.gelu(F.linear(h, tw[q + "mlp.fc1.weight"], tw[q + "mlp.fc1.bias"])), tw[q + "mlp.fc2.weight"], tw[q + "mlp.fc2.bias"])
            t = t + tw[q + "ls2.gamma"] * h
            if i in layers:
                feats.append(F.layer_norm(t, (C,), tw["norm.weight"], tw["norm.bias"], 1e-6)[:, 1:])
        out = []
        for i, f in enumerate(feats):
            f = cl(f.permute(0, 2, 1).reshape(B, C, gh, gw))
            f = F.conv2d(f, hd[f"projects.{i}.weight"], hd[f"projects.{i}.bias"])
            if i < 2:
                f = F.conv_transpose2d(f, hd[f"resize_layers.{i}.weight"], hd[f"resize_layers.{i}.bias"], stride=4 >> i)
            elif i == 3:
                f = F.conv2d(f, hd["resize_layers.3.weight"], hd["resize_layers.3.bias"], stride=2, padding=1)
            out.append(F.conv2d(f, hd[f"scratch.layer{i + 1}_rn.weight"], None, padding=1))
        interp = lambda z, size: F.interpolate(z, size=tuple(size), mode="bilinear", align_corners=True)

        def rcu(q, z):
            c = F.conv2d(F.relu(z), hd[q + "conv1.weight"], hd[q + "conv1.bias"], padding=1)
            return F.conv2d(F.relu(c), hd[q + "conv2.weight"], hd[q + "conv2.bias"], padding=1) + z

        p = None
        for n in (4, 3, 2, 1):
            q = f"scratch.refinenet{n}."
            z = out[n - 1] if p is None else p + rcu(q + "resConfUnit1.", out[n - 1])
            z = rcu(q + "resConfUnit2.", z)
            size = out[n - 2].shape[2:] if n > 1 else (2 * z.shape[2], 2 * z.shape[3])
            p = F.conv2d(interp(z, size), hd[q + "out_conv.weight"], hd[q + "out_conv.bias"])
        c = F.conv2d(p, hd["scratch.output_conv1.weight"], hd["scratch.output_conv1.bias"], padding=1)
        c = interp(c, (14 * gh, 14 * gw))
        y = F.relu(F.conv2d(c, hd["scratch.output_conv2.0.weight"], hd["scratch.output_conv2.0.bias"], padding=1))
        return F.relu(F.conv2d(y, hd["scratch.output_conv2.2.weight"], hd["scratch.output_conv2.2.bias"]))[:, 0].float()
    return run


def measure(size, iters, warmup):
    import torch
    import dpt_ref as R
    from anyedit_amd import _lib, ops
    from anyedit_amd.checkpoints import load_depth_anything
    from anyedit_amd.depth_anything_v2 import DepthAnythingV2, ENCODERS
    torch.manual_seed(0)
    cfg, layers = ENCODERS["vitl"]
    heads = cfg["num_heads"]
    sd = R.seeded_state_dict(cfg, 256, (256, 512, 1024, 1024), seed=1)
    net = DepthAnythingV2("vitl")
    load_depth_anything(net, sd)
    net = net.to("cuda").eval()
    px = R.smooth_pixels(1, size, size, seed=7).to("cuda")
    x = R.normalize(px.cpu()).to("cuda")
    with torch.no_grad():
        net(x)
        y = next(v for k, v in net.depth_head._ws.items())["oc2"]           # output_conv2[0] before its ReLU, rows [H W, 32]
        hw, hb = net.depth_head.scratch.output_conv2[2].weight, net.depth_head.scratch.output_conv2[2].bias
        pre = torch.relu(y.float()) @ hw.view(-1, 1).float() + hb.float()
        R.rescale_tail(sd, pre.cpu())                                       # a depth that is neither flat nor all clipped: last layer rescaled on this image
        load_depth_anything(net, sd)
        depth = net(x).clone()
        clipped, ratio = float((depth == 0).float().mean()), float(depth.std() / depth.mean())
        f_eager = timed(lambda: net(x), iters, warmup)
        d_eager = timed(lambda: net.detect(px), iters, warmup)
        gf = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gf):
            out_f = net(x)
        f_replay = timed(gf.replay, iters, warmup)
        assert torch.equal(out_f, depth)
        rgb = net.detect(px).clone()
        gd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gd):
            out_d = net.detect(px)
        d_replay = timed(gd.replay, iters, warmup)
        assert torch.equal(out_d, rgb)
        ref = torch_bf16_forward(sd, heads, layers)
        theirs = ref(x)
        rel = float((theirs.double() - depth.double()).norm() / depth.double().norm())
        torch_ms = timed(lambda: ref(x), iters, warmup)
        with ops.OpProfiler() as prof:
            for _ in range(iters):
                net.detect(px)
        table = prof.summary(by_shape=True)
    rows = [{"launch": k, "calls_per_detect": v["calls"] // iters, "launches_per_call": v["launches"] // v["calls"], "avg_us": round(v["avg_us"], 2),
             "tflops": round(v["tflops"], 1), "gbps": round(v["gbps"], 1)} for k, v in table.items()]
    total_us = sum(r["avg_us"] * r["calls_per_detect"] for r in rows)
    return {"device": _lib.device_arch(), "geometry": f"Depth Anything V2 ViT-L, features 256, {size}x{size}, B=1", "iters": iters, "warmup": warmup,
            "clipped_share": round(clipped, 3), "std_over_mean": round(ratio, 3),
            "forward_eager_ms": f_eager[0], "forward_eager_min_max_ms": f_eager[1:], "forward_graph_replay_ms": f_replay[0], "forward_graph_min_max_ms": f_replay[1:],
            "detect_eager_ms": d_eager[0], "detect_eager_min_max_ms": d_eager[1:], "detect_graph_replay_ms": d_replay[0], "detect_graph_min_max_ms": d_replay[1:],
            "torch_bf16_forward_ms": torch_ms[0], "torch_bf16_min_max_ms": torch_ms[1:], "vs_torch_bf16_rel_l2": round(rel, 5),
            "sum_of_launches_ms": round(total_us / 1e3, 4), "launches": rows}


def render(res):
    lines = [json.dumps({k: v for k, v in res.items() if k != "launches"})]
    lines.append(f"{'launch':<100} {'calls':>5} {'avg us':>10} {'TFLOP/s':>8} {'GB/s':>8}")
    for r in sorted(res["launches"], key=lambda r: -r["avg_us"] * r["calls_per_detect"]):
        lines.append(f"{r['launch']:<100} {r['calls_per_detect']:>5} {r['avg_us']:>10.2f} {r['tflops']:>8.1f} {r['gbps']:>8.1f}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.size, a.iters, a.warmup)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--iters", str(a.iters),
           "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(f"the measuring process ended with status {r.returncode}; nothing more is started", file=sys.stderr)
        return r.returncode
    text = render(json.loads(r.stdout.strip().splitlines()[-1]))
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
