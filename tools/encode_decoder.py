"""Time of GroundingDINO's language-guided query selection (transformer.py:284-310) on the kernels of csrc/gdino_decoder.hip at production
geometry — the four levels of an 800x800 image (100x100, 50x50, 25x25, 13x13 = 13 294 image tokens), d_model 256, 256 text tokens of which 16
are used, 900 queries, batch 1, seeded inputs — next to its torch form on the same GPU in the same process:

  HIP    proposals kernel; row maximum of the contrastive logits (no [13 294, 256] buffer); stable top-k; gather of 900 rows; the box MLP's
         first two layers (fp32) and its fused last layer + anchor update on the 900 selected rows
  torch  gen_encoder_output_proposals as the reference writes it (about ten launches per level); bf16 matmul + masked_fill + max; torch.topk;
         the box MLP (fp32) on all 13 294 rows; gather

The input of both is the same bf16 `output_memory` rows (enc_output + enc_output_norm are GEMM + LayerNorm on either side and are left out).
Second figure ("forward"): ms per forward of query selection + decoder + heads (`Transformer` without encoder layers + `prediction_heads`) at
6 layers, dim_feedforward 2048, 900 queries, eager and graph replay, next to the same computation on torch's bf16 operators
(`torch_bf16_forward`: the restatement's statements on bf16 GPU tensors; box MLPs and the deformable attention are fp32 on both sides).

    python tools/encode_decoder.py [--iters 20] [--warmup 5] [--step-timeout 300] [--out FILE]

The measurement runs in a child process under `--step-timeout` seconds (this process never opens the GPU).  Each figure is a host clock around
`iters` calls that ends in a device synchronise, after `warmup` untimed calls; the window is repeated 3 times and the median is reported with the
spread.  Eager and graph replay both.  Prints one JSON line.  These are reports, not gates.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS = [(100, 100), (50, 50), (25, 25), (13, 13)]
N_TEXT, N_USED, NQ, C = 256, 16, 900, 256


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


def torch_proposals(mask_d, dev):
    """gen_encoder_output_proposals as the reference states it, in its order (about ten launches per level): mask_d bool [1, N]."""
    import torch
    out, cur = [], 0
    for lvl, (H, W) in enumerate(LEVELS):
        m = mask_d[:, cur:cur + H * W].view(1, H, W, 1)
        vh, vw = torch.sum(~m[:, :, 0, 0], 1), torch.sum(~m[:, 0, :, 0], 1)
        gy, gx = torch.meshgrid(torch.linspace(0, H - 1, H, dtype=torch.float32, device=dev), torch.linspace(0, W - 1, W, dtype=torch.float32, device=dev),
                                indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([vw.unsqueeze(-1), vh.unsqueeze(-1)], 1).view(1, 1, 1, 2)
        grid = (grid.unsqueeze(0) + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** lvl)
        out.append(torch.cat((grid, wh), -1).view(1, -1, 4))
        cur += H * W
    p = torch.cat(out, 1)
    valid = ((p > 0.01) & (p < 0.99)).all(-1, keepdim=True)
    return torch.log(p / (1 - p)).masked_fill(mask_d.unsqueeze(-1), float("inf")).masked_fill(~valid, float("inf"))


def measure(iters, warmup):
    import torch
    import torch.nn.functional as F
    from anyedit_amd import ops
    from anyedit_amd.groundingdino.utils import MLP
    import gdino_dec_ref as R
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    N = sum(h * w for h, w in LEVELS)
    mask = torch.zeros(1, N, dtype=torch.bool)
    s = 0
    for H, W in LEVELS:                                   # the right fifth of every level is padding
        a = torch.zeros(H, W, dtype=torch.bool)
        a[:, W - W // 5:] = True
        mask[0, s:s + H * W] = a.reshape(-1)
        s += H * W
    _, keep_ref = R.encoder_output_proposals(mask, LEVELS)
    mem = torch.randn(1, N, C, generator=g)
    mem = torch.where(keep_ref[..., None], mem, mem[:, :1])   # rows the reference zeroes leave enc_output_norm as ONE row: exact score ties
    mem = mem.to(torch.bfloat16).to(dev)
    text = torch.randn(1, N_TEXT, C, generator=g).to(torch.bfloat16).to(dev)
    tmask = torch.zeros(1, N_TEXT, dtype=torch.bool)
    tmask[:, :N_USED] = True
    tmask, mask_d = tmask.to(dev), mask.to(dev)
    mlp = MLP(C, C, 4, 3)
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.06 if p.dim() == 2 else 0.1))
    mlp = mlp.to(dev)

    def hip():
        prop, _ = ops.gdino_proposals(mask_d, LEVELS)
        _, score = ops.contrastive(mem, text, tmask, max_text_len=N_TEXT, want_logits=False, want_rowmax=True)
        idx = ops.topk_rows(score, NQ).long()
        rows = mem[0].index_select(0, idx[0])
        boxes, unsig = mlp.refine(rows, prop[0].index_select(0, idx[0]), ref_is_logit=True, want_unsigmoid=True)
        return idx, boxes, unsig, score

    torch_proposals = lambda: globals()["torch_proposals"](mask_d, dev)

    L0, L1, L2 = mlp.layers

    def torch_form():
        prop = torch_proposals()
        logits = (mem @ text.transpose(-1, -2)).float().masked_fill(~tmask[:, None, :], float("-inf"))
        score = logits.max(-1)[0]
        x = mem.float()
        delta = F.linear(F.relu(F.linear(F.relu(F.linear(x, L0.weight, L0.bias)), L1.weight, L1.bias)), L2.weight, L2.bias)
        unsig_all = delta + prop
        idx = torch.topk(score, NQ, dim=1)[1]
        unsig = torch.gather(unsig_all, 1, idx.unsqueeze(-1).repeat(1, 1, 4))
        return idx, unsig.sigmoid(), unsig, score

    with torch.no_grad():
        h, t = hip(), torch_form()
        torch.cuda.synchronize()
        same_set = len(set(h[0][0].tolist()) & set(t[0][0].tolist()))
        score_rel = float((h[3] - t[3]).double().norm() / t[3].double().norm())
        stable = bool(torch.equal(h[0].cpu(), R.stable_topk(h[3].cpu(), NQ)))
        eager, t_eager = timed(hip, iters, warmup), timed(torch_form, iters, warmup)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                hip()
            replay = timed(graph.replay, iters, warmup)
            try:
                tgraph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(tgraph):
                    torch_form()
                t_replay = timed(tgraph.replay, iters, warmup)
            except RuntimeError as e:                      # the torch form is the yardstick only: report that it could not be captured
                print(f"torch form not captured: {e}", file=sys.stderr)
                t_replay = None
        parts = {"proposals_ms": timed(lambda: ops.gdino_proposals(mask_d, LEVELS), iters, warmup)[0],
                 "rowmax_ms": timed(lambda: ops.contrastive(mem, text, tmask, max_text_len=N_TEXT, want_logits=False, want_rowmax=True), iters, warmup)[0],
                 "topk_ms": timed(lambda: ops.topk_rows(h[3], NQ), iters, warmup)[0],
                 "torch_proposals_ms": timed(torch_proposals, iters, warmup)[0],
                 "torch_topk_ms": timed(lambda: torch.topk(t[3], NQ, dim=1), iters, warmup)[0]}
    r = lambda v: round(v, 4)
    return dict({"what": "query selection, 13294 image tokens, 256 text tokens (16 used), 900 queries, batch 1; host clock", "iters": iters,
                 "eager_ms": r(eager[0]), "eager_min_max_ms": [r(eager[1]), r(eager[2])], "graph_replay_ms": r(replay[0]),
                 "graph_min_max_ms": [r(replay[1]), r(replay[2])], "torch_eager_ms": r(t_eager[0]), "torch_eager_min_max_ms": [r(t_eager[1]), r(t_eager[2])],
                 "torch_graph_replay_ms": t_replay and r(t_replay[0]), "torch_graph_min_max_ms": t_replay and [r(t_replay[1]), r(t_replay[2])],
                 "hip_over_torch_graph": t_replay and r(replay[0] / t_replay[0]), "hip_over_torch_eager": r(eager[0] / t_eager[0]),
                 "selected_in_common_with_torch_topk": same_set, "scores_rel_l2_vs_torch_bf16": score_rel, "selection_is_the_stable_sort_of_its_scores": stable},
                **{k: r(v) for k, v in parts.items()})


def torch_bf16_forward(m, sd, dev="cuda"):
    """Query selection + decoder + heads on torch's bf16 operators (tests/gdino_dec_ref.py's statements on bf16 GPU tensors): F.linear, LayerNorm,
    F.scaled_dot_product_attention, bf16 matmul + masked_fill + max, torch.topk, the proposals as the reference writes them.  fp32 on both sides:
    every box MLP (on ALL rows in the selection, as the reference runs it) and the deformable attention, which runs the module's own path."""
    import torch
    import torch.nn.functional as F
    import gdino_dec_ref as R
    bf = torch.bfloat16
    w = {k: v.to(dev, bf) for k, v in sd.items()}
    f = {k: v.to(dev).float() for k, v in sd.items() if "bbox_embed" in k}
    ln = lambda x, p: F.layer_norm(x, x.shape[-1:], w[p + ".weight"], w[p + ".bias"], 1e-5)
    lin = lambda x, p: F.linear(x, w[p + ".weight"], w[p + ".bias"])
    C, H, nl = 256, 8, len(m.decoder.layers)
    period = torch.tensor(10000.0, device=dev) ** (2.0 * torch.floor(torch.arange(128, device=dev) / 2.0) / 128.0)
    even = (torch.arange(128, device=dev) % 2) == 0

    def mlp32(x, p):
        for i in range(3):
            x = F.linear(x, f[f"{p}layers.{i}.weight"], f[f"{p}layers.{i}.bias"])
            x = F.relu(x) if i < 2 else x
        return x

    def sine(boxes):
        out = []
        for c in (1, 0, 2, 3):
            ang = boxes[..., c, None] * (2.0 * math.pi) / period
            out.append(torch.where(even, ang.sin(), ang.cos()))
        return torch.cat(out, -1).to(bf)

    def run(srcs, masks, text, tmask, shapes_dev, starts_dev):
        mem = torch.cat([x.flatten(2).transpose(1, 2) for x in srcs], 1).to(bf)
        kpm = torch.cat([k.flatten(1) for k in masks], 1)
        B, N, _ = mem.shape
        vr = torch.stack([torch.stack([(~k[:, 0, :]).sum(1).float() / k.shape[2], (~k[:, :, 0]).sum(1).float() / k.shape[1]], -1) for k in masks], 1)
        t = text.to(bf)
        prop = torch_proposals(kpm, dev)
        keep = torch.isfinite(prop).all(-1, keepdim=True)
        om = ln(lin(mem * keep, "enc_output"), "enc_output_norm")
        score = (om @ t.transpose(-1, -2)).float().masked_fill(~tmask[:, None, :], float("-inf")).max(-1)[0]
        unsig_all = mlp32(om.float(), "enc_out_bbox_embed.") + prop
        idx = torch.topk(score, NQ, dim=1)[1]
        unsig = torch.gather(unsig_all, 1, idx.unsqueeze(-1).repeat(1, 1, 4))
        x = w["tgt_embed.weight"][None].expand(B, -1, -1)
        nq = x.shape[1]
        ref = unsig.sigmoid()
        memf = mem.float().reshape(B * N, C)
        sp = lambda u, n: u.view(B, n, H, C // H).transpose(1, 2)
        un = lambda a, n: a.transpose(1, 2).reshape(B, n, C)
        tlive = tmask[:, None, None, :]
        refs = [ref]
        for l in range(nl):
            p = f"decoder.layers.{l}."
            rpi = R.reference_points_input(ref, vr)
            qpos = lin(F.relu(lin(sine(rpi[:, :, 0, :]), "decoder.ref_point_head.layers.0")), "decoder.ref_point_head.layers.1")
            W, b = w[p + "self_attn.in_proj_weight"], w[p + "self_attn.in_proj_bias"]
            qk = x + qpos
            a = F.scaled_dot_product_attention(sp(F.linear(qk, W[:C], b[:C]), nq), sp(F.linear(qk, W[C:2 * C], b[C:2 * C]), nq), sp(F.linear(x, W[2 * C:], b[2 * C:]), nq))
            y = ln(x + lin(un(a, nq), p + "self_attn.out_proj"), p + "norm2")
            W, b = w[p + "ca_text.in_proj_weight"], w[p + "ca_text.in_proj_bias"]
            Nt = t.shape[1]
            a = F.scaled_dot_product_attention(sp(F.linear(y + qpos, W[:C], b[:C]), nq), sp(F.linear(t, W[C:2 * C], b[C:2 * C]), Nt), sp(F.linear(t, W[2 * C:], b[2 * C:]), Nt),
                                               attn_mask=tlive)
            y = ln(y + lin(un(a, nq), p + "ca_text.out_proj"), p + "catext_norm")
            d = m.decoder.layers[l]._deform((y.float() + qpos.float()).reshape(B * nq, C), rpi, memf, shapes_dev, starts_dev, kpm, B, nq, N).view(B, nq, C)
            y = ln((y.float() + d).to(bf), p + "norm1")
            x = ln(y + lin(F.relu(lin(y, p + "linear1")), p + "linear2"), p + "norm3")
            ref = (mlp32(x.float(), f"decoder.bbox_embed.{l}.") + R.inverse_sigmoid(ref)).sigmoid()
            refs.append(ref)
        h = ln(x, "decoder.norm")
        boxes = (mlp32(h.float(), f"decoder.bbox_embed.{nl - 1}.") + R.inverse_sigmoid(refs[-2])).sigmoid()
        logits = (h @ t.transpose(-1, -2)).float().masked_fill(~tmask[:, None, :], float("-inf"))
        return {"pred_logits": logits, "pred_boxes": boxes, "selected": idx}

    return run


def measure_forward(iters, warmup):
    """Query selection + decoder + heads at production geometry (6 layers, dim_feedforward 2048, 900 queries; the enhancer's output stands in as
    `srcs`, so no encoder layer runs): ms per forward, eager and graph replay, next to `torch_bf16_forward` on the same inputs."""
    import torch
    from anyedit_amd.groundingdino.transformer import Transformer, prediction_heads
    from anyedit_amd.groundingdino.utils import MLP, ContrastiveEmbed
    import gdino_enc_ref as E
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(1)
    m = Transformer(d_model=C, nhead=8, num_queries=NQ, num_encoder_layers=0, num_decoder_layers=6, dim_feedforward=2048, dropout=0.0, return_intermediate_dec=True,
                    num_feature_levels=4, learnable_tgt_init=True, two_stage_type="standard", embed_init_tgt=True, use_text_cross_attention=True)
    m.decoder.bbox_embed = torch.nn.ModuleList([MLP(C, C, 4, 3)] * 6)
    m.decoder.class_embed = torch.nn.ModuleList([ContrastiveEmbed()] * 6)
    m.enc_out_bbox_embed, m.enc_out_class_embed = MLP(C, C, 4, 3), ContrastiveEmbed()
    sd = E.draw_weights(m.state_dict(), g)
    for k in list(sd):
        if "bbox_embed" in k and k.endswith("layers.2.weight"):
            sd[k] = sd[k] * 0.1
    m.load_state_dict(sd)
    m = m.eval().requires_grad_(False).to(dev)
    srcs, masks, poss = [], [], []
    for H, W in LEVELS:
        srcs.append(torch.randn(1, C, H, W, generator=g).to(dev))
        poss.append(torch.zeros(1, C, H, W, device=dev))
        a = torch.zeros(1, H, W, dtype=torch.bool)
        a[:, :, W - W // 5:] = True
        masks.append(a.to(dev))
    text = torch.randn(1, N_TEXT, C, generator=g).to(dev)
    tmask = torch.zeros(1, N_TEXT, dtype=torch.bool)
    tmask[:, :N_USED] = True
    tmask = tmask.to(dev)

    def fwd():
        td = {"encoded_text": text, "text_token_mask": tmask}
        hs, refs, _, _, _ = m(srcs, masks, None, poss, None, None, td)
        return prediction_heads(hs, refs, m.decoder.bbox_embed, m.decoder.class_embed, td)

    ref = torch_bf16_forward(m, sd)
    with torch.no_grad():
        out = fwd()
        ref_call = lambda: ref(srcs, masks, text, tmask, m.decoder.__dict__["_shapes_dev"], m.__dict__["_starts_dev"])   # device copies of the eager forward
        tout = ref_call()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(out["pred_boxes"]).all())
        sel = m.last_topk_proposals
        common = len(set(sel[0].tolist()) & set(tout["selected"][0].tolist()))
        same_slots = sel == tout["selected"]
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        box_rel = rel(out["pred_boxes"][same_slots], tout["pred_boxes"][same_slots]) if bool(same_slots.any()) else None
        eager, t_eager = timed(fwd, iters, warmup), timed(ref_call, iters, warmup)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        t_replay = None
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fwd()
            replay = timed(graph.replay, iters, warmup)
            try:
                tgraph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(tgraph):
                    ref_call()
                t_replay = timed(tgraph.replay, iters, warmup)
            except RuntimeError as e:                      # the torch form is the yardstick only: report that it could not be captured
                print(f"torch bf16 forward not captured: {e}", file=sys.stderr)
    r = lambda v: round(v, 4)
    return {"what": "query selection + decoder (6 layers, dff 2048) + heads, 13294 image tokens, 256 text tokens (16 used), 900 queries, batch 1; host clock",
            "iters": iters, "eager_ms": r(eager[0]), "eager_min_max_ms": [r(eager[1]), r(eager[2])], "graph_replay_ms": r(replay[0]),
            "graph_min_max_ms": [r(replay[1]), r(replay[2])], "boxes_finite": finite,
            "torch_bf16_eager_ms": r(t_eager[0]), "torch_bf16_eager_min_max_ms": [r(t_eager[1]), r(t_eager[2])],
            "torch_bf16_graph_replay_ms": t_replay and r(t_replay[0]), "torch_bf16_graph_min_max_ms": t_replay and [r(t_replay[1]), r(t_replay[2])],
            "hip_over_torch_eager": r(eager[0] / t_eager[0]), "hip_over_torch_graph": t_replay and r(replay[0] / t_replay[0]),
            "selected_in_common_with_torch": common, "slots_with_the_same_index": int(same_slots.sum()),
            "pred_boxes_rel_l2_on_those_slots": box_rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps({"selection": measure(a.iters, a.warmup), "forward": measure_forward(a.iters, a.warmup)}), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--one", "--iters", str(a.iters), "--warmup", str(a.warmup)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
    if res.returncode != 0:
        print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
        print(f"the measuring process ended with status {res.returncode}", file=sys.stderr)
        return res.returncode
    line = res.stdout.strip().split("\n")[-1]
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
