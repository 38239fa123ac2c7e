"""Time of one HED edge map (hed.HEDdetector.detect: what the `visual_scribble` condition costs per image), reference geometry (13 convolutions,
64 .. 512 channels), seeded weights with the heads rescaled on the image, one 512x512 uint8 image: eager (launch-per-op from Python) and as a
replayed graph, next to the same network on torch's own bf16 operators (channels-last F.conv2d / relu / max_pool2d, fp32 F.interpolate), and
the per-launch table of one eager detect (HIP events around every launch: stem, 12 convolutions, 7 ReLUs, 5 tails, fuse).

    python tools/encode_scribble.py [--iters 200] [--warmup 20] [--size 512] [--step-timeout 300] [--out FILE]

The measurement runs in a child process of its own under `--step-timeout` seconds (this process never opens the GPU); if it fails or runs out
of time nothing else is started.  Each figure is a host clock around `iters` calls that ends in a device synchronise, after `warmup` untimed
calls; the window is repeated 3 times and the median is reported with the spread.  Arithmetic of the network at 512x512: about 174 GFLOP, 33 MB
per full-resolution 64-channel bf16 map.
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


def torch_bf16_detect(sd, layers):
    """The same network and detector arithmetic on torch's operators: bf16 channels-last convolutions, fp32 projections' resize, fp64 sigmoid."""
    import torch
    import torch.nn.functional as F
    bf = lambda t: t.to("cuda", torch.bfloat16)
    p = {k: (bf(v).contiguous(memory_format=torch.channels_last) if v.dim() == 4 and "convs" in k else bf(v)) for k, v in sd.items()}
    norm = sd["norm"].to("cuda")

    def run(image_u8):
        B, H, W, _ = image_u8.shape
        h = (image_u8.permute(0, 3, 1, 2).float() - norm).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        maps = []
        for n, l in enumerate(layers, 1):
            if n > 1:
                h = F.max_pool2d(h, 2, 2)
            for m in range(l):
                h = F.relu(F.conv2d(h, p[f"block{n}.convs.{m}.weight"], p[f"block{n}.convs.{m}.bias"], padding=1))
            maps.append(F.interpolate(F.conv2d(h, p[f"block{n}.projection.weight"], p[f"block{n}.projection.bias"]).float(), size=(H, W), mode="bilinear",
                                      align_corners=False))
        v = (255.0 / (1.0 + torch.exp(-torch.stack(maps, 0).mean(0)[:, 0].double()))).clamp(0.0, 255.0).to(torch.uint8)
        return 255 - v
    return run


def measure(size, iters, warmup):
    import torch
    import hed_ref as R
    from anyedit_amd import _lib, ops
    from anyedit_amd.hed import HEDdetector
    torch.manual_seed(0)
    img = R.smooth_image(size, size, seed=7)
    sd = R.seeded_state_dict(seed=1)
    det = HEDdetector(sd, device="cuda")
    static = torch.from_numpy(img).unsqueeze(0).to("cuda")
    with torch.no_grad():
        sides = det.netNetwork.side_maps(static)
        R.rescale_heads(sd, [s.unsqueeze(1).cpu() for s in sides], size, size)       # an unsaturated map: heads rescaled on this image
        det.netNetwork.load_state_dict(sd)
        edge, logit = det.detect(static, want_logits=True)
        unsat = float(((edge > 5) & (edge < 250)).float().mean())
        eager = timed(lambda: det.detect(static), iters, warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = det.detect(static)
        replay = timed(graph.replay, iters, warmup)
        assert torch.equal(out, edge)
        ref = torch_bf16_detect(sd, det.netNetwork.layers)
        theirs = ref(static)
        d = (theirs.int() - edge.int()).abs()
        torch_ms = timed(lambda: ref(static), iters, warmup)
        with ops.OpProfiler() as prof:
            for _ in range(iters):
                det.detect(static)
        table = prof.summary(by_shape=True)
    rows = [{"launch": k, "calls_per_detect": v["calls"] // iters, "launches_per_call": v["launches"] // v["calls"], "avg_us": round(v["avg_us"], 2),
             "tflops": round(v["tflops"], 1), "gbps": round(v["gbps"], 1)} for k, v in table.items()]
    total_us = sum(r["avg_us"] * r["calls_per_detect"] for r in rows)
    return {"device": _lib.device_arch(), "geometry": f"HED 64..512 channels, 13 convolutions, {size}x{size} uint8, B=1", "iters": iters, "warmup": warmup,
            "logit_std": round(float(logit.std()), 3), "unsaturated_share": round(unsat, 3),
            "eager_ms": eager[0], "eager_min_max_ms": eager[1:], "graph_replay_ms": replay[0], "graph_min_max_ms": replay[1:],
            "torch_bf16_ms": torch_ms[0], "torch_bf16_min_max_ms": torch_ms[1:],
            "vs_torch_bf16_uint8_max_diff": int(d.max()), "vs_torch_bf16_uint8_differing_share": round(float((d > 0).float().mean()), 4),
            "sum_of_launches_ms": round(total_us / 1e3, 4), "launches": rows}


def render(res):
    lines = [json.dumps({k: v for k, v in res.items() if k != "launches"})]
    lines.append(f"{'launch':<100} {'calls':>5} {'avg us':>10} {'TFLOP/s':>8} {'GB/s':>8}")
    for r in sorted(res["launches"], key=lambda r: -r["avg_us"] * r["calls_per_detect"]):
        lines.append(f"{r['launch']:<100} {r['calls_per_detect']:>5} {r['avg_us']:>10.2f} {r['tflops']:>8.1f} {r['gbps']:>8.1f}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--step-timeout", type=int, default=300)
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
