"""Time of one CLIP vision encode (CLIPVisionModelWithProjection.encode_pixels(px, -2): what train.py:689-691 feeds the adapter), ViT-H/14
geometry (224 px, 257 tokens, 31 of 32 layers), seeded weights, at B = 1 / 4 images: eager (launch-per-op from Python) and as a replayed graph.

    python tools/encode_image.py [--iters 50] [--warmup 10] [--batches 1 4] [--step-timeout 240] [--out FILE]

Every batch size is measured in a child process of its own under `--step-timeout` seconds (this process never opens the GPU); the first child
that fails or runs out of time ends the run, nothing else is started after it.  Each figure is a host clock around `iters` encodes that ends
in a device synchronise (the clock is read after the synchronise), after `warmup` untimed encodes of the same shape; the window is repeated
3 times and the median is reported with the spread.  Prints one JSON line per batch size.
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


def measure(B, iters, warmup):
    import torch
    import clip_vision_ref
    from anyedit_amd import _lib
    from anyedit_amd.ldm.modules.encoders.clip_vision import CLIPVisionModelWithProjection, CLIP_VIT_H_14_VISION as cfg
    sd = clip_vision_ref.seeded_state_dict(cfg, seed=0)
    with torch.device("meta"):
        m = CLIPVisionModelWithProjection()
    m.load_state_dict(sd, assign=True)
    m = m.to("cuda")
    px = torch.randn(B, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(1)).to("cuda")
    with torch.no_grad():
        eager = timed(lambda: m.encode_pixels(px), iters, warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.encode_pixels(px)
        replay = timed(graph.replay, iters, warmup)
        assert torch.isfinite(out.float()).all()
    return {"device": _lib.device_arch(), "geometry": "ViT-H/14 vision, 224 px, 257 tokens, hidden_states[-2]", "B": B, "iters": iters, "warmup": warmup,
            "eager_ms": round(eager[0], 4), "eager_min_max_ms": [round(eager[1], 4), round(eager[2], 4)],
            "graph_replay_ms": round(replay[0], 4), "graph_min_max_ms": [round(replay[1], 4), round(replay[2], 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help="(internal) measure this batch size in this process")
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(measure(a.one, a.iters, a.warmup)), flush=True)
        return 0
    lines = []
    for B in a.batches:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(B), "--iters", str(a.iters),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"B={B}: the measuring process ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
