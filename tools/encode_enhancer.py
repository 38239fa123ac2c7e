"""Time of one forward of GroundingDINO's feature enhancer (groundingdino/transformer.py: what the detector of tools/tool.py runs on the backbone's
maps and the text features), production geometry (d_model 256, 8 heads, dim_feedforward 2048, 6 layers, 4 points), the four levels of an 800x800
image (100x100, 50x50, 25x25, 13x13 = 13 294 image tokens), 256 and 16 text tokens, seeded weights, batch 1: eager (launch-per-op from Python) and
as a replayed graph — and next to it the yardstick: the same enhancer run by torch's own bf16 operators on the same GPU in the same process
(tests/gdino_enc_ref.py's statements on bf16 tensors; its deformable attention keeps the module's fp32 path, so that term is the same on both
sides) — and the time of the fusion attention alone (`ops.bi_attention`: three launches) against the reference's bmm / softmax form on bf16
tensors at the same shape.

    python tools/encode_enhancer.py [--iters 10] [--warmup 3] [--layers 6] [--text 256 16] [--step-timeout 500] [--out FILE]

The measurement runs in a child process under `--step-timeout` seconds (this process never opens the GPU).  Each figure is a host clock around
`iters` calls that ends in a device synchronise (the clock is read after the synchronise), after `warmup` untimed calls of the same shape; the
window is repeated 3 times and the median is reported with the spread.  The per-launch times of the fusion attention are such host-clock
figures too, not a kernel trace.  Prints one JSON line per text length.  These are reports, not gates.
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

LEVELS = [(100, 100), (50, 50), (25, 25), (13, 13)]


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


def torch_fusion_attention(q, k, vv, vl, heads, scale):
    """BiMultiHeadAttention's bmm / softmax form (no masks) on bf16 tensors [B, N, heads D]: materialises [B heads, Nv, Nt] as the reference does."""
    import torch
    B, Nv, C = q.shape
    Nt, D = k.shape[1], C // heads
    sp = lambda t, n: t.view(B, n, heads, D).transpose(1, 2).reshape(B * heads, n, D)
    Q, K, VV, VL = sp(q, Nv), sp(k, Nt), sp(vv, Nv), sp(vl, Nt)
    S = torch.bmm(Q * scale, K.transpose(1, 2))
    S = S - S.max()
    St = S.transpose(1, 2)
    Pl = (St - St.max(-1, keepdim=True)[0]).softmax(-1)
    Pv = S.softmax(-1)
    ov, ol = torch.bmm(Pv, VL), torch.bmm(Pl, VV)
    un = lambda t, n: t.view(B, heads, n, D).transpose(1, 2).reshape(B, n, C)
    return un(ov, Nv), un(ol, Nt)


def torch_bf16_enhancer(sd, cfg, sizes):
    """The enhancer on torch's bf16 operators (no padding masks): LayerNorm, F.linear, bmm / softmax fusion, F.scaled_dot_product_attention for the
    text layer, bf16 everywhere except the deformable attention, which runs the module's own fp32 path on both sides."""
    import torch
    import torch.nn.functional as F
    bf = torch.bfloat16
    w = {k: v.to("cuda", bf) for k, v in sd.items()}
    nl, nhead = cfg["num_layers"], cfg["nhead"]
    ln = lambda x, p: F.layer_norm(x, x.shape[-1:], w[p + ".weight"], w[p + ".bias"], 1e-5)
    lin = lambda x, p: F.linear(x, w[p + ".weight"], w[p + ".bias"])

    def run(m, src, pos, ref_pts, shapes, starts, text, pos_text, allowed_bh):
        x, t = src.to(bf), text.to(bf)
        B, Nv, C = x.shape
        Nt, H = t.shape[1], nhead // 2
        pt = pos_text.to(bf)
        for i in range(nl):
            p = f"fusion_layers.{i}."
            vn, tn = ln(x, p + "layer_norm_v"), ln(t, p + "layer_norm_l")
            ov, ol = torch_fusion_attention(lin(vn, p + "attn.v_proj"), lin(tn, p + "attn.l_proj"), lin(vn, p + "attn.values_v_proj"),
                                            lin(tn, p + "attn.values_l_proj"), H, (w[p + "attn.v_proj.weight"].shape[0] // H) ** -0.5)
            x = vn + w[p + "gamma_v"] * lin(ov, p + "attn.out_v_proj")
            t = tn + w[p + "gamma_l"] * lin(ol, p + "attn.out_l_proj")
            p = f"text_layers.{i}."
            qk = t + pt
            W, b = w[p + "self_attn.in_proj_weight"], w[p + "self_attn.in_proj_bias"]
            sp = lambda u: u.view(B, Nt, H, C // H).transpose(1, 2)
            a = F.scaled_dot_product_attention(sp(F.linear(qk, W[:C], b[:C])), sp(F.linear(qk, W[C:2 * C], b[C:2 * C])), sp(F.linear(t, W[2 * C:], b[2 * C:])),
                                               attn_mask=allowed_bh)
            y = ln(t + lin(a.transpose(1, 2).reshape(B, Nt, C), p + "self_attn.out_proj"), p + "norm1")
            t = ln(y + lin(F.relu(lin(y, p + "linear1")), p + "linear2"), p + "norm2")
            p = f"layers.{i}."
            d = m.layers[i]._deform(x.reshape(B * Nv, C), pos.reshape(B * Nv, C), ref_pts, shapes, starts, None, B, Nv).view(B, Nv, C)
            y = ln((x.float() + d).to(bf), p + "norm1")
            x = ln(y + lin(F.relu(lin(y, p + "linear1")), p + "linear2"), p + "norm2")
        return x.float(), t.float()

    return run


def measure(n_text, layers, iters, warmup):
    import torch
    import gdino_enc_ref as R
    from anyedit_amd import _lib, ops
    from anyedit_amd.groundingdino.transformer import build_feature_enhancer
    from anyedit_amd.groundingdino.transformer_vanilla import expand_text_mask
    gen = torch.Generator().manual_seed(0)
    m = build_feature_enhancer(num_layers=layers)
    sd = R.draw_weights(m.state_dict(), gen)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    B, C, Nv = 1, 256, sum(h * w for h, w in LEVELS)
    starts = [0]
    for h, w in LEVELS[:-1]:
        starts.append(starts[-1] + h * w)
    cut = max(1, n_text // 3)
    tsam = torch.eye(n_text, dtype=torch.bool)[None].clone()
    for lo in range(0, n_text, cut):
        tsam[0, lo:lo + cut, lo:lo + cut] = True
    ids = (torch.arange(n_text) % cut)[None]
    dev = lambda t: t.to("cuda")
    inp = dict(src=dev(torch.randn(B, Nv, C, generator=gen)), pos=dev(0.5 * torch.randn(B, Nv, C, generator=gen)), spatial_shapes=dev(torch.tensor(LEVELS)),
               level_start_index=dev(torch.tensor(starts)), valid_ratios=dev(torch.ones(B, 4, 2)), key_padding_mask=None,
               memory_text=dev(torch.randn(B, n_text, C, generator=gen)), text_attention_mask=None, text_self_attention_masks=dev(tsam), position_ids=dev(ids))
    ref = torch_bf16_enhancer(sd, dict(num_layers=layers, nhead=8), LEVELS)
    ref_pts = m.get_reference_points(LEVELS, inp["valid_ratios"], "cuda")
    pos_text = R.sine_pos_embed(ids[..., None], 256, exchange_xy=False).to("cuda")
    allowed_bh = expand_text_mask(inp["text_self_attention_masks"], 4).bool().view(B, 4, n_text, n_text)
    ref_call = lambda: ref(m, inp["src"], inp["pos"], ref_pts, inp["spatial_shapes"], inp["level_start_index"], inp["memory_text"], pos_text, allowed_bh)
    r = lambda v: round(v, 4)
    with torch.no_grad():
        eager = timed(lambda: m(**inp), iters, warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = m(**inp)
        replay = timed(graph.replay, iters, warmup)
        t_eager = timed(ref_call, iters, warmup)
        tgraph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(tgraph):
            touts = ref_call()
        t_replay = timed(tgraph.replay, iters, warmup)
        torch.cuda.synchronize()
        agree = [r(float((a - b).norm() / b.norm())) for a, b in zip(outs, touts)]
        assert all(torch.isfinite(a).all() for a in outs)
        # the fusion attention alone at the production shape: 4 heads x 256
        E, heads = 1024, 4
        bf = torch.bfloat16
        q, vv = (torch.randn(B, Nv, E, generator=gen).to("cuda", bf) for _ in range(2))
        k, vl = (torch.randn(B, n_text, E, generator=gen).to("cuda", bf) for _ in range(2))
        ov, ol = torch.empty_like(q), torch.empty_like(k)
        t_hip = timed(lambda: ops.bi_attention(q, k, vv, vl, heads, 0.0625, out_v=ov, out_l=ol), 4 * iters, warmup)
        t_torch = timed(lambda: torch_fusion_attention(q, k, vv, vl, heads, 0.0625), 4 * iters, warmup)
        tv, tl = torch_fusion_attention(q, k, vv, vl, heads, 0.0625)
        fa = [r(float((ov.float() - tv.float()).norm() / tv.float().norm())), r(float((ol.float() - tl.float()).norm() / tl.float().norm()))]
    return {"device": _lib.device_arch(), "geometry": f"d_model 256, 8 heads, dff 2048, {layers} layers, levels {LEVELS} = {Nv} image tokens, {n_text} text tokens, batch 1",
            "iters": iters, "warmup": warmup, "eager_ms": r(eager[0]), "eager_min_max_ms": [r(eager[1]), r(eager[2])],
            "graph_replay_ms": r(replay[0]), "graph_min_max_ms": [r(replay[1]), r(replay[2])],
            "torch_bf16_eager_ms": r(t_eager[0]), "torch_bf16_eager_min_max_ms": [r(t_eager[1]), r(t_eager[2])],
            "torch_bf16_graph_replay_ms": r(t_replay[0]), "torch_bf16_graph_min_max_ms": [r(t_replay[1]), r(t_replay[2])],
            "hip_over_torch_graph": r(replay[0] / t_replay[0]), "hip_over_torch_eager": r(eager[0] / t_eager[0]), "rel_l2_hip_vs_torch_bf16": agree,
            "fusion_attention": {"shape": f"{Nv} x {n_text} tokens, 4 heads x 256", "partials": -(-Nv // ops.bi_attention_split_rows(Nv)),
                                 "hip_three_launches_ms": r(t_hip[0]), "hip_min_max_ms": [r(t_hip[1]), r(t_hip[2])],
                                 "torch_bmm_softmax_ms": r(t_torch[0]), "torch_min_max_ms": [r(t_torch[1]), r(t_torch[2])],
                                 "hip_over_torch": r(t_hip[0] / t_torch[0]), "per_forward_hip_ms": r(t_hip[0] * layers), "per_forward_torch_ms": r(t_torch[0] * layers),
                                 "rel_l2_hip_vs_torch": fa, "clock": "host clock around the launches ending in a device synchronise; no kernel trace"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--text", type=int, nargs="+", default=[256, 16])
    ap.add_argument("--step-timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help="(internal) measure this text length in this process")
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(measure(a.one, a.layers, a.iters, a.warmup)), flush=True)
        return 0
    lines = []
    for n_text in a.text:           # one child per text length; a child that fails ends the run
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(n_text), "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--layers", str(a.layers)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"the measuring process for {n_text} text tokens ended with status {res.returncode}", file=sys.stderr)
            return res.returncode
        lines.append(res.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
