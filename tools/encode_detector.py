"""Time of the GroundingDINO detector (anyedit_amd/groundingdino/groundingdino.py) at production geometry — Swin-B-384 (window 12, stages 1-3
out), BERT-base, six enhancer and six decoder layers, 900 queries, four levels — with seeded random weights, one 800x800 image (levels 100x100,
50x50, 25x25, 13x13 = 13 294 tokens) and a 9-token caption:

  forward   ms per `GroundingDINO.detect` (token ids already on the GPU), eager and graph replay
  neck      the four input_proj levels (ops.gemm / ops.conv3x3 with fp32 output + ae_gdino_neck_groupnorm into src_flatten) and the one launch of
            ae_gdino_level_geometry, next to the torch form of the same on bf16 operators in the same process: F.conv2d + F.group_norm on the
            NCHW maps, flatten / transpose / cat, F.interpolate of the mask, the sine embedding as position_encoding.py:98-131 states it,
            + level_embed, get_valid_ratio
  ground    ae_gdino_ground + the read-back of its rows, next to "copy the [900, 256] logits to the host and filter there" (tools/tool.py:125-133)

    python tools/encode_detector.py [--iters 10] [--warmup 3] [--step-timeout 600] [--out FILE]

The measurement runs in a child process under `--step-timeout` seconds (this process never opens the GPU).  Each figure is a host clock around
`iters` calls that ends in a device synchronise, after `warmup` untimed calls; the window is repeated 3 times and the median is reported with the
spread.  Prints one JSON line.  These are reports, not gates.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 800
CAPTION_IDS = [101, 4937, 1012, 2417, 3899, 1012, 3242, 1012, 102]      # [CLS] w . w w . w . [SEP]: 9 tokens, three phrases


class FixedTokenizer:
    """The caption above, whatever the text: the timing needs ids, not a vocabulary file."""

    def convert_tokens_to_ids(self, tokens):
        return [101, 102, 1012, 1029]

    def __call__(self, captions, padding="longest", return_tensors="pt"):
        import torch
        ids = torch.tensor([CAPTION_IDS for _ in captions])
        return {"input_ids": ids, "attention_mask": torch.ones_like(ids), "token_type_ids": torch.zeros_like(ids)}


def swinb_args():
    return types.SimpleNamespace(
        backbone="swin_B_384_22k", position_embedding="sine", pe_temperatureH=20, pe_temperatureW=20, return_interm_indices=[1, 2, 3],
        backbone_freeze_keywords=None, hidden_dim=256, dropout=0.0, nheads=8, num_queries=900, dim_feedforward=2048, enc_layers=6, dec_layers=6,
        pre_norm=False, query_dim=4, transformer_activation="relu", num_patterns=0, num_feature_levels=4, enc_n_points=4, dec_n_points=4,
        two_stage_type="standard", embed_init_tgt=True, use_text_enhancer=True, use_fusion_layer=True, use_checkpoint=True, use_transformer_ckpt=True,
        use_text_cross_attention=True, text_dropout=0.0, fusion_dropout=0.0, fusion_droppath=0.1, dec_pred_bbox_embed_share=True,
        two_stage_bbox_embed_share=False, two_stage_class_embed_share=False, dn_box_noise_scale=1.0, dn_label_noise_ratio=0.5, dn_labelbook_size=2000,
        text_encoder_type="bert-base-uncased", sub_sentence_present=True, max_text_len=256)


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
    return dict(ms=round(ms[len(ms) // 2], 4), min=round(ms[0], 4), max=round(ms[-1], 4))


def graphed(fn, iters, warmup):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
    torch.cuda.synchronize()
    return timed(g.replay, iters, warmup)


def torch_neck(maps, mask, proj, level_embed, tH, tW):
    """groundingdino.py:291-310 + transformer.py:226-246 on bf16 operators: maps bf16 NCHW per backbone level, mask bool [B, H, W]."""
    import torch
    import torch.nn.functional as F
    srcs = [p(x) for p, x in zip(proj, maps)]
    for p in proj[len(maps):]:
        srcs.append(p(maps[-1] if len(srcs) == len(maps) else srcs[-1]))
    src_f, mask_f, pos_f, vrs = [], [], [], []
    i = torch.arange(128, dtype=torch.float32, device=mask.device)
    dim_tx = tW ** (2 * torch.div(i, 2, rounding_mode="floor") / 128)
    dim_ty = tH ** (2 * torch.div(i, 2, rounding_mode="floor") / 128)
    for l, s in enumerate(srcs):
        m = F.interpolate(mask[None].float(), size=s.shape[-2:]).to(torch.bool)[0]
        nm = ~m
        y_embed, x_embed = nm.cumsum(1, dtype=torch.float32), nm.cumsum(2, dtype=torch.float32)
        y_embed = y_embed / (y_embed[:, -1:, :] + 1e-6) * (2 * math.pi)
        x_embed = x_embed / (x_embed[:, :, -1:] + 1e-6) * (2 * math.pi)
        px, py = x_embed[..., None] / dim_tx, y_embed[..., None] / dim_ty
        px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=4).flatten(3)
        py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=4).flatten(3)
        pos = torch.cat((py, px), dim=3).flatten(1, 2) + level_embed[l].view(1, 1, -1)
        src_f.append(s.flatten(2).transpose(1, 2))
        mask_f.append(m.flatten(1))
        pos_f.append(pos.to(torch.bfloat16))
        _, h, w = m.shape
        vrs.append(torch.stack([torch.sum(~m[:, 0, :], 1).float() / w, torch.sum(~m[:, :, 0], 1).float() / h], -1))
    return torch.cat(src_f, 1), torch.cat(mask_f, 1), torch.cat(pos_f, 1), torch.stack(vrs, 1)


def measure(iters, warmup):
    import copy
    import torch
    from anyedit_amd.groundingdino import inference as I
    from anyedit_amd.groundingdino.groundingdino import build_groundingdino
    dev = "cuda:0"
    torch.manual_seed(0)
    m = build_groundingdino(swinb_args(), tokenizer=FixedTokenizer()).eval().requires_grad_(False).to(dev)
    g = torch.Generator().manual_seed(1)
    px = torch.randn(1, 3, H, W, generator=g).to(dev)
    mask = torch.zeros(1, H, W, dtype=torch.bool)
    mask[:, 700:, :], mask[:, :, 760:] = True, True
    mask = mask.to(dev)
    tok = {k: v.to(dev) for k, v in FixedTokenizer()(["x"]).items()}
    tok["attention_mask"] = tok["attention_mask"].bool()
    res = {"geometry": dict(image=[H, W], levels=m.level_sizes(H, W), tokens=sum(h * w for h, w in m.level_sizes(H, W)), caption_tokens=len(CAPTION_IDS))}

    fwd = lambda: m.detect(px, mask, tok)
    out = fwd()
    res["forward"] = dict(eager=timed(fwd, iters, warmup), graph=graphed(fwd, iters, warmup))

    tower = m.backbone[0]
    tws = tower.run(px)
    hip_neck = lambda: m.neck(tws.stages, mask, 1, H, W)
    maps = [tws.stages[i].out.to(torch.bfloat16) for i in range(tower.num_layers) if i in tower.out_indices]
    proj = copy.deepcopy(m.input_proj).to(torch.bfloat16)
    le = m.transformer.level_embed.detach().float()
    pe = m.backbone[1]
    t_neck = lambda: torch_neck(maps, mask, proj, le, pe.temperatureH, pe.temperatureW)
    ws = hip_neck()
    ts, tm, tp, tv = t_neck()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    res["neck"] = dict(hip=dict(eager=timed(hip_neck, iters, warmup), graph=graphed(hip_neck, iters, warmup)),
                       torch_bf16=dict(eager=timed(t_neck, iters, warmup), graph=graphed(t_neck, iters, warmup)),
                       agreement=dict(src_rel_l2=rel(ws.src, ts), pos_rel_l2=rel(ws.pos, tp), mask_equal=bool(torch.equal(ws.mask, tm)),
                                      valid_ratios_max_abs_diff=float((ws.vr - tv).abs().max())))

    logits, boxes = out["pred_logits"].contiguous(), out["pred_boxes"].contiguous()
    logits = torch.where(torch.isfinite(logits), torch.randn(logits.shape, device=dev) * 2 - 1.5, logits)     # the zero-initialised heads give one value

    def hip_ground():
        return I.ground_outputs(logits, boxes, 0.3, 0.25)

    def host_ground():
        lg = logits.cpu().sigmoid()[0]
        bx = boxes.cpu()[0]
        filt = lg.max(dim=1)[0] > 0.3
        return lg[filt] > 0.25, bx[filt]

    a, b = hip_ground()[0], host_ground()
    res["ground"] = dict(hip=timed(hip_ground, iters, warmup), host_filter=timed(host_ground, iters, warmup), kept=int(a[0].numel()),
                         same_boxes=bool(torch.equal(a[2], b[1])), same_posmaps=bool(torch.equal(a[3], b[0])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.iters, a.warmup)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--one", "--iters", str(a.iters), "--warmup", str(a.warmup)]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.step_timeout)
    except subprocess.TimeoutExpired:
        print(f"the measuring process did not end within {a.step_timeout} s", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
        print(f"the measuring process ended with status {res.returncode}", file=sys.stderr)
        return 1
    line = res.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
