"""Time of one pass of the `visual_segment` annotator (uniformer.upernet.EncoderDecoder: UniFormer-S backbone, UPerHead with channels 512, 150
classes), seeded weights, one 512x512 image, next to the same network on torch's own bf16 operators; the per-launch table of one eager pass; the
segment-map kernel alone against torch's resize, softmax and argmax on the same logits; the two large convolutions' FLOP/s from their shapes.

    python tools/encode_segment.py [--iters 20] [--warmup 5] [--size 512] [--step-timeout 300] [--out FILE]

Each step (`model`, `launches`, `argmax`, `convs`) runs in a child process of its own under `--step-timeout` seconds (this process never opens the
GPU); if one fails or runs out of time nothing else is started.  Each figure is a host clock around `iters` calls that ends in a device synchronise,
after `warmup` untimed calls; the window is repeated 3 times and the median is reported with the spread.  The HIP and the torch pass alternate window
by window on the same device.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEPS = ("model", "launches", "argmax", "convs")
HBM_ATTAINABLE_TBPS = 6.3     # a float4 copy on MI355X (8.0 TB/s specified)


def window(fn, iters):
    import torch
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def timed_alternating(fns, iters, warmup, windows=3):
    """{name: [median, min, max] ms}; one window of each function in turn, `windows` times"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ms[k].append(window(fn, iters))
    return {k: [round(v, 4) for v in (sorted(m)[len(m) // 2], min(m), max(m))] for k, m in ms.items()}


def build(size):
    import torch
    import uniformer_ref as UR
    import upernet_ref as R
    from anyedit_amd.checkpoints import load_segmentor
    from anyedit_amd.uniformer import UniFormer
    from anyedit_amd.uniformer.upernet import EncoderDecoder, UPerHead
    geo, hg = UR.S_GEOMETRY, R.WIDE_HEAD
    bsd = UR.seeded_state_dict(geo["layers"], geo["embed_dim"], geo["head_dim"], seed=1)
    hsd = R.seeded_head_state_dict(seed=2, **hg)
    pal = torch.randint(0, 256, (150, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).numpy()
    model = EncoderDecoder(UniFormer(), UPerHead(pool_scales=hg["pool_scales"], in_channels=list(hg["in_channels"]), channels=hg["channels"], num_classes=150,
                                                norm_cfg=dict(type="BN")), test_cfg=dict(mode="whole"), palette=pal)
    load_segmentor(model, dict({"backbone." + k: v for k, v in bsd.items()}, **{"decode_head." + k: v for k, v in hsd.items()}))
    return model.to("cuda"), bsd, hsd, UR.smooth_pixels(1, size, size, seed=7).to("cuda")


def torch_bf16_head(hsd, pool_scales):
    """The head on torch's operators: bf16 weights (the BatchNorm folded as the HIP path folds it) and activations, channels-last maps, fp32 logits"""
    import torch
    import torch.nn.functional as F
    import upernet_ref as R
    bf = torch.bfloat16
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    mods = {}
    for k in hsd:
        if k.endswith("conv.weight"):
            q = k[:-len("conv.weight")]
            w, b = R.fold_bn_after_conv(hsd[k], *[hsd[q + "bn." + n] for n in ("weight", "bias", "running_mean", "running_var")])
            mods[q] = (cl(w.to("cuda", bf)), b.to("cuda", bf))
    wseg, bseg = cl(hsd["conv_seg.weight"].to("cuda", bf)), hsd["conv_seg.bias"].to("cuda", bf)
    cm = lambda q, t: F.relu(F.conv2d(t, *mods[q], padding=mods[q][0].shape[-1] // 2))
    rs = lambda t, size: F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=False)

    def run(maps):
        maps = [cl(m.to(bf)) for m in maps]
        x = maps[3]
        outs = [x] + [rs(cm(f"psp_modules.{k}.1.", F.adaptive_avg_pool2d(x, s)), x.shape[2:]) for k, s in enumerate(pool_scales)]
        lat = [cm(f"lateral_convs.{i}.", maps[i]) for i in range(3)] + [cm("bottleneck.", torch.cat(outs, 1))]
        for i in range(3, 0, -1):
            lat[i - 1] = lat[i - 1] + rs(lat[i], lat[i - 1].shape[2:])
        fpn = [cm(f"fpn_convs.{i}.", lat[i]) for i in range(3)] + [lat[3]]
        cat = torch.cat([fpn[0]] + [rs(f, fpn[0].shape[2:]) for f in fpn[1:]], 1)
        return F.conv2d(cm("fpn_bottleneck.", cat), wseg, bseg).float()
    return run


def torch_tail(logits, size):
    """encode_decode's resize (whole_inference's is the identity here), inference's softmax and simple_test's argmax, as the reference runs them"""
    import torch.nn.functional as F
    return F.softmax(F.interpolate(logits, size=size, mode="bilinear", align_corners=False), dim=1).argmax(dim=1)


def step_model(size, iters, warmup):
    import torch
    import uniformer_ref as UR
    import upernet_ref as R
    from anyedit_amd import _lib
    from encode_segment_backbone import torch_bf16_forward
    model, bsd, hsd, x = build(size)
    with torch.no_grad():
        hip = lambda: model.simple_test(x, want_colours=True)
        labels, colours = [t.clone() for t in hip()]
        rows, h, w = model.encode_decode_rows(x)
        logits = rows[:, :150].reshape(1, h, w, 150).permute(0, 3, 1, 2).float().contiguous()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = hip()
        backbone, head = torch_bf16_forward(bsd, UR.S_GEOMETRY["head_dim"]), torch_bf16_head(hsd, R.WIDE_HEAD["pool_scales"])
        theirs = lambda: torch_tail(head(backbone(x)), (size, size))
        their_logits = head(backbone(x))
        their_labels = theirs()
        ms = timed_alternating({"hip_eager": hip, "hip_graph": graph.replay, "torch_bf16": theirs}, iters, warmup)
        assert torch.equal(out[0], labels) and torch.equal(out[1], colours)
    return {"device": _lib.device_arch(), "geometry": f"UniFormer-S + UPerHead(512), 150 classes, {size}x{size}, B=1; image -> labels and colours",
            "iters": iters, "warmup": warmup, "hip_eager_ms": ms["hip_eager"], "hip_graph_replay_ms": ms["hip_graph"], "torch_bf16_ms": ms["torch_bf16"],
            "ms_are": "[median, min, max] of 3 alternating windows", "logits_std": round(float(logits.std()), 3),
            "logits_rel_l2_hip_vs_torch_bf16": round(float((their_logits.double() - logits.double()).norm() / logits.double().norm()), 5),
            "share_of_equal_labels": round(float((their_labels == labels.long()).float().mean()), 5), "distinct_labels": int(labels.unique().numel())}


def step_launches(size, iters, warmup):
    import torch
    from anyedit_amd import ops
    model, _, _, x = build(size)
    with torch.no_grad():
        for _ in range(warmup):
            model.simple_test(x, want_colours=True)
        with ops.OpProfiler() as prof:
            for _ in range(iters):
                model.simple_test(x, want_colours=True)
        table = prof.summary(by_shape=True)
    rows = [{"launch": k, "calls": v["calls"] // iters, "launches_per_call": v["launches"] // v["calls"], "avg_us": round(v["avg_us"], 2),
             "tflops": round(v["tflops"], 1), "gbps": round(v["gbps"], 1)} for k, v in table.items()]
    return {"launches_per_pass": sum(r["calls"] * r["launches_per_call"] for r in rows),
            "sum_of_launches_ms": round(sum(r["avg_us"] * r["calls"] for r in rows) / 1e3, 4), "launches": rows}


def step_argmax(size, iters, warmup):
    """ae_seg_argmax_u8 alone on logits [size/4, size/4, 152] (150 classes) -> size x size: algorithmic bytes (logits once, labels and colours once)
    per second, and its time against torch's resize + softmax + argmax on the same logits (NCHW fp32, as the reference holds them)"""
    import torch
    from anyedit_amd import ops
    h = size // 4
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = torch.randn(h * h, 152, device="cuda", generator=g) * 5
    nchw = rows[:, :150].reshape(1, h, h, 150).permute(0, 3, 1, 2).contiguous()
    pal = torch.randint(0, 256, (150, 3), device="cuda", dtype=torch.uint8)
    lab, col = torch.empty(1, size, size, dtype=torch.uint8, device="cuda"), torch.empty(1, size, size, 3, dtype=torch.uint8, device="cuda")
    ms = timed_alternating({"hip": lambda: ops.seg_argmax(rows, 150, 1, h, h, (size, size), palette=pal, labels=lab, colours=col),
                            "hip_two_stages": lambda: ops.seg_argmax(rows, 150, 1, h, h, (size, size), (size - 29, size + 37), palette=pal),
                            "torch": lambda: torch_tail(nchw, (size, size))}, iters, warmup)
    agree = float((torch_tail(nchw, (size, size)) == lab.long()).float().mean())
    nbytes = 4 * h * h * 150 + size * size * 4
    return {"argmax_alone": {"shape": f"{h}x{h}x150 -> {size}x{size}", "hip_ms": ms["hip"], "hip_two_stages_ms": ms["hip_two_stages"], "torch_resize_softmax_argmax_ms": ms["torch"],
                             "algorithmic_MiB": round(nbytes / 2 ** 20, 2), "hip_TBps": round(nbytes / (ms["hip"][0] * 1e-3) / 1e12, 4),
                             "share_of_attainable": round(nbytes / (ms["hip"][0] * 1e-3) / 1e12 / HBM_ATTAINABLE_TBPS, 4), "labels_equal_to_torch": round(agree, 6)}}


def step_convs(size, iters, warmup):
    """fpn_bottleneck (3x3, 2048 -> 512) and fpn_convs[0] (3x3, 512 -> 512) on the stride-4 map: FLOP/s from the shapes"""
    import torch
    from anyedit_amd import ops
    h = size // 4
    out = []
    for name, cin in (("fpn_bottleneck", 2048), ("fpn_convs.0", 512)):
        g = torch.Generator(device="cuda").manual_seed(cin)
        x = torch.randn(h * h, cin, device="cuda", generator=g).to(torch.bfloat16)
        w = ops.pack_conv3x3(torch.randn(512, cin, 3, 3, device="cuda", generator=g) / (3 * cin ** 0.5))
        b = torch.zeros(512, device="cuda")
        ms = timed_alternating({"conv": lambda: ops.conv3x3(x, w, b, 1, h, h)}, iters, warmup)["conv"]
        flop = 2.0 * h * h * 512 * 9 * cin
        out.append({"conv": f"{name}: 3x3 {cin} -> 512 on {h}x{h}", "ms": ms, "GFLOP": round(flop / 1e9, 1), "TFLOPs": round(flop / (ms[0] * 1e-3) / 1e12, 1),
                    "plan": ops.plan_label(ops.conv_plan(1, h, h, cin, 512))})
    return {"convs_alone": out}


def render(res):
    lines = [json.dumps({k: v for k, v in res.items() if k not in ("launches", "argmax_alone", "convs_alone")})]
    if "launches" in res:
        lines.append(f"{'launch':<110} {'calls':>5} {'avg us':>10} {'TFLOP/s':>8} {'GB/s':>8}")
        for r in sorted(res["launches"], key=lambda r: -r["avg_us"] * r["calls"]):
            lines.append(f"{r['launch']:<110} {r['calls']:>5} {r['avg_us']:>10.2f} {r['tflops']:>8.1f} {r['gbps']:>8.1f}")
    if "argmax_alone" in res:
        lines.append(f"segment-map kernel alone (algorithmic bytes; attainable {HBM_ATTAINABLE_TBPS} TB/s): " + json.dumps(res["argmax_alone"]))
    for r in res.get("convs_alone", []):
        lines.append("convolution alone: " + json.dumps(r))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=STEPS, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(globals()["step_" + a.child](a.size, a.iters, a.warmup)), flush=True)
        return 0
    res = {}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step, "--size", str(a.size), "--iters", str(a.iters),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    text = render(res)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
