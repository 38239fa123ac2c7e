"""Time of one DINOv2 reference encode (FrozenDinoV2Encoder.encode_pixels: what visual_reference_tool.py:203 feeds AnyDoor's cross-attention),
ViT-g/14 geometry (224 px, 257 tokens, 40 blocks, projector to 1024), seeded weights, at B = 1 / 2 images: eager (launch-per-op from Python) and
as a replayed graph — and next to it the yardstick: the same encoder run by torch's own bf16 operators on the same GPU in the same process
(tests/dino_ref.py's statements on bf16 tensors: F.conv2d, F.layer_norm, F.linear, F.scaled_dot_product_attention, F.silu), eager and replayed.

    python tools/encode_reference.py [--iters 30] [--warmup 5] [--batches 1 2] [--depth 40] [--step-timeout 300] [--out FILE]

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


def torch_bf16_encoder(sd, cfg, pos):
    """The encoder on torch's bf16 operators: weights, activations and the position table bf16 on the GPU."""
    import torch
    import torch.nn.functional as F
    import dino_ref
    w = {k: v.to("cuda", torch.bfloat16) for k, v in sd.items()}
    C, heads, L, P = cfg["embed_dim"], cfg["num_heads"], cfg["depth"], cfg["patch_size"]
    mean = torch.tensor(dino_ref.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(dino_ref.IMAGENET_STD, device="cuda").view(1, 3, 1, 1)
    pos = pos.to("cuda", torch.bfloat16)
    eps = cfg["layer_norm_eps"]

    def run(px):
        x = ((px - mean) / std).to(torch.bfloat16)
        B = x.shape[0]
        patch = F.conv2d(x, w["model.patch_embed.proj.weight"], w["model.patch_embed.proj.bias"], stride=P).flatten(2).transpose(1, 2)
        x = torch.cat([w["model.cls_token"].expand(B, 1, C), patch], 1) + pos
        N = x.shape[1]
        sp = lambda t: t.view(B, N, heads, C // heads).transpose(1, 2)
        for i in range(L):
            q = f"model.blocks.{i}."
            h = F.layer_norm(x, (C,), w[q + "norm1.weight"], w[q + "norm1.bias"], eps)
            qq, kk, vv = F.linear(h, w[q + "attn.qkv.weight"], w[q + "attn.qkv.bias"]).split(C, dim=-1)
            o = F.scaled_dot_product_attention(sp(qq), sp(kk), sp(vv)).transpose(1, 2).reshape(B, N, C)
            x = x + w[q + "ls1.gamma"] * F.linear(o, w[q + "attn.proj.weight"], w[q + "attn.proj.bias"])
            h = F.layer_norm(x, (C,), w[q + "norm2.weight"], w[q + "norm2.bias"], eps)
            x1, x2 = F.linear(h, w[q + "mlp.w12.weight"], w[q + "mlp.w12.bias"]).chunk(2, dim=-1)
            x = x + w[q + "ls2.gamma"] * F.linear(F.silu(x1) * x2, w[q + "mlp.w3.weight"], w[q + "mlp.w3.bias"])
        x = F.layer_norm(x, (C,), w["model.norm.weight"], w["model.norm.bias"], eps)
        return F.linear(x, w["projector.weight"], w["projector.bias"])

    return run


def measure(B, iters, warmup, depth):
    import torch
    import dino_ref
    from anyedit_amd import _lib
    from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder, DINOV2_VITG14, interpolated_pos_embed
    cfg = dict(DINOV2_VITG14, depth=depth)
    sd = dino_ref.seeded_state_dict(cfg, seed=0, projector_out=1024)
    with torch.device("meta"):
        m = FrozenDinoV2Encoder(cfg)
    m.load_state_dict(sd, assign=True)
    m = m.to("cuda")
    px = torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to("cuda")
    ref = torch_bf16_encoder(sd, cfg, interpolated_pos_embed(sd["model.pos_embed"], 16, 16, cfg["interpolate_offset"]))
    with torch.no_grad():
        eager = timed(lambda: m.encode_pixels(px), iters, warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.encode_pixels(px)
        replay = timed(graph.replay, iters, warmup)
        t_eager = timed(lambda: ref(px), iters, warmup)
        tgraph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(tgraph):
            tout = ref(px)
        t_replay = timed(tgraph.replay, iters, warmup)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all() and torch.isfinite(tout.float()).all()
        agree = float((out.float() - tout.float()).norm() / tout.float().norm())
    r = lambda v: round(v, 4)
    return {"device": _lib.device_arch(), "geometry": f"DINOv2 ViT-g/14, 224 px, 257 tokens, {depth} blocks, projector 1024", "B": B, "iters": iters,
            "warmup": warmup, "eager_ms": r(eager[0]), "eager_min_max_ms": [r(eager[1]), r(eager[2])],
            "graph_replay_ms": r(replay[0]), "graph_min_max_ms": [r(replay[1]), r(replay[2])],
            "torch_bf16_eager_ms": r(t_eager[0]), "torch_bf16_eager_min_max_ms": [r(t_eager[1]), r(t_eager[2])],
            "torch_bf16_graph_replay_ms": r(t_replay[0]), "torch_bf16_graph_min_max_ms": [r(t_replay[1]), r(t_replay[2])],
            "hip_over_torch_graph": r(replay[0] / t_replay[0]), "hip_over_torch_eager": r(eager[0] / t_eager[0]), "rel_l2_hip_vs_torch_bf16": r(agree)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--depth", type=int, default=40)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help="(internal) measure this batch size in this process")
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(measure(a.one, a.iters, a.warmup, a.depth)), flush=True)
        return 0
    lines = []
    for B in a.batches:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(B), "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--depth", str(a.depth)]
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
