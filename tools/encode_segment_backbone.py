"""Time of one pass of the `visual_segment` annotator's backbone (uniformer.UniFormer at the UniFormer-S geometry: layers 3 / 4 / 8 / 3, widths
64 / 128 / 320 / 512, head dim 64), seeded weights, one 512x512 image: `forward` (the four fp32 NCHW maps) eager (launch-per-op from Python) and as
a replayed graph, next to the same network on torch's own bf16 operators (channels-last F.conv2d for the patch, depthwise and 1x1 convolutions,
F.batch_norm, F.layer_norm, F.linear, scaled_dot_product_attention), the per-launch table of one eager forward (HIP events around every launch),
and the depthwise kernel alone on maps large enough to leave the caches (bytes moved per second against the attainable HBM rate).

    python tools/encode_segment_backbone.py [--iters 20] [--warmup 5] [--size 512] [--step-timeout 420] [--out FILE]

The measurement runs in a child process of its own under `--step-timeout` seconds (this process never opens the GPU); if it fails or runs out of
time nothing else is started.  Each figure is a host clock around `iters` calls that ends in a device synchronise, after `warmup` untimed calls; the
window is repeated 3 times and the median is reported with the spread.
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
HBM_ATTAINABLE_TBPS = 6.3     # a float4 copy on MI355X (8.0 TB/s specified)


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


def torch_bf16_forward(sd, head_dim):
    """The same network on torch's operators: bf16 weights and activations (channels-last maps), the operators' own accumulation, fp32 outputs."""
    import torch
    import torch.nn.functional as F
    import uniformer_ref as R
    bf = torch.bfloat16
    cl = lambda t: t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
    p = {k: cl(v.to("cuda", bf)) for k, v in sd.items() if v.is_floating_point()}
    layers = R.layers_of(sd)

    def ln(x, q, eps):
        return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), p[q + "weight"], p[q + "bias"], eps).permute(0, 3, 1, 2)

    def bn(x, q):
        return F.batch_norm(x, p[q + "running_mean"], p[q + "running_var"], p[q + "weight"], p[q + "bias"], False, 0.0, 1e-5)

    def cblock(q, x):
        C = x.shape[1]
        x = x + F.conv2d(x, p[q + "pos_embed.weight"], p[q + "pos_embed.bias"], padding=1, groups=C)
        t = F.conv2d(bn(x, q + "norm1."), p[q + "conv1.weight"], p[q + "conv1.bias"])
        t = F.conv2d(t, p[q + "attn.weight"], p[q + "attn.bias"], padding=2, groups=C)
        x = x + F.conv2d(t, p[q + "conv2.weight"], p[q + "conv2.bias"])
        t = F.gelu(F.conv2d(bn(x, q + "norm2."), p[q + "mlp.fc1.weight"], p[q + "mlp.fc1.bias"]))
        return x + F.conv2d(t, p[q + "mlp.fc2.weight"], p[q + "mlp.fc2.bias"])

    def sablock(q, x):
        B, C, H, W = x.shape
        heads = C // head_dim
        x = x + F.conv2d(x, p[q + "pos_embed.weight"], p[q + "pos_embed.bias"], padding=1, groups=C)
        t = x.flatten(2).transpose(1, 2)
        y = F.layer_norm(t, (C,), p[q + "norm1.weight"], p[q + "norm1.bias"], 1e-6)
        qkv = F.linear(y, p[q + "attn.qkv.weight"], p[q + "attn.qkv.bias"]).view(B, H * W, 3, heads, head_dim).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B, H * W, C)
        t = t + F.linear(o, p[q + "attn.proj.weight"], p[q + "attn.proj.bias"])
        y = F.layer_norm(t, (C,), p[q + "norm2.weight"], p[q + "norm2.bias"], 1e-6)
        t = t + F.linear(F.gelu(F.linear(y, p[q + "mlp.fc1.weight"], p[q + "mlp.fc1.bias"])), p[q + "mlp.fc2.weight"], p[q + "mlp.fc2.bias"])
        return t.transpose(1, 2).reshape(B, C, H, W)

    def run(x):
        h = cl(x.to(bf))
        outs = []
        for n, depth in enumerate(layers, 1):
            q = f"patch_embed{n}."
            h = ln(F.conv2d(h, p[q + "proj.weight"], p[q + "proj.bias"], stride=4 if n == 1 else 2), q + "norm.", 1e-5)
            for i in range(depth):
                h = (cblock if n <= 2 else sablock)(f"blocks{n}.{i}.", h)
            outs.append(ln(h, f"norm{n}.", 1e-6).float().contiguous())
        return tuple(outs)
    return run


def dwconv_alone(iters, warmup):
    """The depthwise kernel on maps of 64 MiB (beyond every cache but the Infinity Cache's reach of the previous launch's output is avoided by
    rotating four input / output pairs): algorithmic bytes (x once, out once, a separate residual once) per second."""
    import torch
    from anyedit_amd import ops
    rows = []
    for (B, H, W, C, k, res) in ((8, 256, 256, 64, 3, "x"), (8, 256, 256, 64, 5, None), (8, 128, 128, 256, 5, None), (8, 128, 128, 320, 3, "x")):
        g = torch.Generator(device="cuda").manual_seed(k)
        xs = [torch.randn(B * H * W, C, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4)]
        outs = [torch.empty_like(x) for x in xs]
        w, b = torch.randn(k * k, C, device="cuda", generator=g) / k, torch.randn(C, device="cuda", generator=g)
        state = {"i": 0}

        def call():
            i = state["i"] = (state["i"] + 1) % 4
            ops.dwconv(xs[i], w, b, B, H, W, residual=xs[i] if res == "x" else None, out=outs[i])
        ms = timed(call, iters, warmup)
        nbytes = 2 * xs[0].numel() * 2
        rows.append({"shape": f"B={B} {H}x{W} C={C} k={k}{' res=x' if res else ''}", "ms": ms[0], "min_max_ms": ms[1:], "MiB_moved": round(nbytes / 2 ** 20, 1),
                     "TBps": round(nbytes / (ms[0] * 1e-3) / 1e12, 3), "share_of_attainable": round(nbytes / (ms[0] * 1e-3) / 1e12 / HBM_ATTAINABLE_TBPS, 3)})
    return rows


def measure(size, iters, warmup):
    import torch
    import uniformer_ref as R
    from anyedit_amd import _lib, ops
    from anyedit_amd.checkpoints import load_uniformer
    from anyedit_amd.uniformer import UniFormer
    torch.manual_seed(0)
    geo = R.S_GEOMETRY
    sd = R.seeded_state_dict(geo["layers"], geo["embed_dim"], geo["head_dim"], seed=1)
    net = UniFormer()
    load_uniformer(net, sd)
    net = net.to("cuda")
    x = R.smooth_pixels(1, size, size, seed=7).to("cuda")
    with torch.no_grad():
        maps = [m.clone() for m in net(x)]
        eager = timed(lambda: net(x), iters, warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(x)
        replay = timed(graph.replay, iters, warmup)
        assert all(torch.equal(a, b) for a, b in zip(out, maps))
        ref = torch_bf16_forward(sd, geo["head_dim"])
        theirs = ref(x)
        rel = [round(float((t.double() - m.double()).norm() / m.double().norm()), 5) for t, m in zip(theirs, maps)]
        torch_ms = timed(lambda: ref(x), iters, warmup)
        with ops.OpProfiler() as prof:
            for _ in range(iters):
                net(x)
        table = prof.summary(by_shape=True)
        alone = dwconv_alone(iters, warmup)
    rows = [{"launch": k, "calls_per_forward": v["calls"] // iters, "launches_per_call": v["launches"] // v["calls"], "avg_us": round(v["avg_us"], 2),
             "tflops": round(v["tflops"], 1), "gbps": round(v["gbps"], 1)} for k, v in table.items()]
    total_us = sum(r["avg_us"] * r["calls_per_forward"] for r in rows)
    return {"device": _lib.device_arch(), "geometry": f"UniFormer-S backbone, {size}x{size}, B=1", "iters": iters, "warmup": warmup,
            "output_std": [round(float(m.std()), 3) for m in maps],
            "forward_eager_ms": eager[0], "forward_eager_min_max_ms": eager[1:], "forward_graph_replay_ms": replay[0], "forward_graph_min_max_ms": replay[1:],
            "torch_bf16_forward_ms": torch_ms[0], "torch_bf16_min_max_ms": torch_ms[1:], "vs_torch_bf16_rel_l2_per_level": rel,
            "launches_per_forward": sum(r["calls_per_forward"] * r["launches_per_call"] for r in rows), "sum_of_launches_ms": round(total_us / 1e3, 4),
            "hbm_attainable_TBps": HBM_ATTAINABLE_TBPS, "dwconv_alone": alone, "launches": rows}


def render(res):
    lines = [json.dumps({k: v for k, v in res.items() if k not in ("launches", "dwconv_alone")})]
    lines.append(f"{'launch':<100} {'calls':>5} {'avg us':>10} {'TFLOP/s':>8} {'GB/s':>8}")
    for r in sorted(res["launches"], key=lambda r: -r["avg_us"] * r["calls_per_forward"]):
        lines.append(f"{r['launch']:<100} {r['calls_per_forward']:>5} {r['avg_us']:>10.2f} {r['tflops']:>8.1f} {r['gbps']:>8.1f}")
    lines.append(f"depthwise kernel alone, maps beyond the caches (algorithmic bytes; attainable {res['hbm_attainable_TBps']} TB/s):")
    for r in res["dwconv_alone"]:
        lines.append("  " + json.dumps(r))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
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
