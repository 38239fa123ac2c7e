"""Time of GroundingDINO's text side (`GroundingDINOText.encode_tokenized`: sub-sentence spans, BERT-base, feat_map) at production geometry —
BERT-base (12 layers, 12 heads of 64, hidden 768, intermediate 3072; the word table cut to 1024 rows), hidden_dim 256, seeded weights —
for captions of 9 and 256 tokens at B = 1 and B = 4, next to torch's bf16 operator form of the same layers on the same GPU in the same process:

  HIP    ops.gdino_text_spans; ops.bert_embed_ln; per layer ops.gemm x 4, ops.attention_span_short, ops.layernorm x 2, ops.bias_act; feat_map
  torch  the masks taken as given (a precomputed bool [B, 1, N, N]); embedding gathers + F.layer_norm; per layer F.linear x 4,
         F.scaled_dot_product_attention under that mask, F.layer_norm x 2, F.gelu; F.linear for feat_map — bf16 weights and activations

Second figure ("attention"): the attention launch alone at 12 heads — `ops.attention_span_short` on the spans against
`ops.attention_masked_short` on the mask expanded to [B*12, N, N], and the expansion itself (what a caller of the dense kernel pays per call).

    python tools/encode_caption.py [--iters 20] [--warmup 5] [--step-timeout 300] [--out FILE]

The measurement runs in a child process under `--step-timeout` seconds (this process never opens the GPU).  Each figure is a host clock around
`iters` calls that ends in a device synchronise, after `warmup` untimed calls; the window is repeated 3 times and the median is reported.  Eager
and graph replay both.  Prints one JSON line.  These are reports, not gates.
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

BASE = dict(vocab_size=1024, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=512,
            type_vocab_size=2)
SPECIAL = [1, 2, 3, 4]
HIDDEN_DIM = 256


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
    return ms[len(ms) // 2]


def caption_ids(B, N, gen):
    """[CLS], phrases of 1 .. 4 words closed by ".", [SEP] on the last column: every sample its own phrase lengths."""
    import torch
    ids = torch.randint(10, BASE["vocab_size"], (B, N), generator=gen)
    ids[:, 0], ids[:, -1] = 1, 2
    for b in range(B):
        n = 1
        while n < N - 1:
            n += int(torch.randint(1, 5, (1,), generator=gen))
            if n < N - 1:
                ids[b, n] = 3
            n += 1
    return ids


def torch_bf16_form(sd, dev):
    import torch
    import torch.nn.functional as F
    bf = torch.bfloat16
    w = {k: v.to(dev, bf) for k, v in sd.items()}
    C, H, L = BASE["hidden_size"], BASE["num_attention_heads"], BASE["num_hidden_layers"]
    ln = lambda x, p: F.layer_norm(x, (C,), w[p + ".weight"], w[p + ".bias"], 1e-12)
    lin = lambda x, p: F.linear(x, w[p + ".weight"], w[p + ".bias"])
    wqkv = [torch.cat([w[f"bert.encoder.layer.{i}.attention.self.{n}.weight"] for n in ("query", "key", "value")], 0) for i in range(L)]
    bqkv = [torch.cat([w[f"bert.encoder.layer.{i}.attention.self.{n}.bias"] for n in ("query", "key", "value")], 0) for i in range(L)]

    def run(ids, pos, mask4):
        B, N = ids.shape
        e = "bert.embeddings."
        x = ln(w[e + "word_embeddings.weight"][ids] + w[e + "position_embeddings.weight"][pos] + w[e + "token_type_embeddings.weight"][0], e + "LayerNorm")
        sp = lambda t: t.view(B, N, H, C // H).transpose(1, 2)
        for i in range(L):
            p = f"bert.encoder.layer.{i}."
            q, k, v = F.linear(x, wqkv[i], bqkv[i]).split(C, -1)
            a = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=mask4).transpose(1, 2).reshape(B, N, C)
            y = ln(x + lin(a, p + "attention.output.dense"), p + "attention.output.LayerNorm")
            x = ln(y + lin(F.gelu(lin(y, p + "intermediate.dense")), p + "output.dense"), p + "output.LayerNorm")
        return lin(x, "feat_map")

    return run


def measure(iters, warmup):
    import torch
    from anyedit_amd import ops
    from anyedit_amd.checkpoints import load_groundingdino_text
    from anyedit_amd.groundingdino.groundingdino import GroundingDINOText
    import bert_ref as R
    dev = "cuda:0"
    sd = R.seeded_state_dict(BASE, HIDDEN_DIM, seed=3)
    m = GroundingDINOText(BASE, hidden_dim=HIDDEN_DIM, special_token_ids=SPECIAL)
    load_groundingdino_text(m, sd)
    m = m.eval().requires_grad_(False).to(dev)
    tform = torch_bf16_form(sd, dev)
    C, H = BASE["hidden_size"], BASE["num_attention_heads"]
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    r = lambda v: round(v, 4)
    rows = []
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for N in (9, 256):
            for B in (1, 4):
                ids = caption_ids(B, N, gen).to(dev)
                tok = {"input_ids": ids, "attention_mask": torch.ones(B, N, dtype=torch.bool, device=dev), "token_type_ids": torch.zeros_like(ids)}
                hip = lambda: m.encode_tokenized(tok)
                td = hip()
                pos, mask4 = td["position_ids"].clone(), td["text_self_attention_masks"][:, None].clone()
                ref = lambda: tform(ids, pos, mask4)
                agree = rel(td["encoded_text"].float(), ref().float())
                eager, t_eager = timed(hip, iters, warmup), timed(ref, iters, warmup)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        hip()
                    replay = timed(graph.replay, iters, warmup)
                    try:
                        tgraph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(tgraph):
                            ref()
                        t_replay = timed(tgraph.replay, iters, warmup)
                    except RuntimeError as e:                  # the torch form is the yardstick only: report that it could not be captured
                        print(f"torch bf16 form not captured: {e}", file=sys.stderr)
                        t_replay = None
                torch.cuda.current_stream().wait_stream(side)
                # the attention launch alone, 12 heads, on a packed q | k | v of this shape
                qkv = torch.randn(B * N, 3 * C, generator=gen).to(torch.bfloat16).to(dev)
                spans, _, dense = ops.gdino_text_spans(ids, SPECIAL, want_mask=True)
                st = (N * 3 * C, 64, 3 * C)
                out = torch.empty(B, N, C, dtype=torch.bfloat16, device=dev)
                big = dense[:, None].expand(B, H, N, N).reshape(B * H, N, N).contiguous().view(torch.uint8)
                span_ms = timed(lambda: ops.attention_span_short(qkv, qkv[:, C:], qkv[:, 2 * C:], spans, B, H, N, 64, 0.125, st, st, st, out=out), iters, warmup)
                a = out.clone()
                dense_ms = timed(lambda: ops.attention_masked_short(qkv, qkv[:, C:], qkv[:, 2 * C:], big, B, H, N, 64, 0.125, st, st, st, out=out), iters, warmup)
                same = bool(torch.equal(a, out))
                expand_ms = timed(lambda: dense[:, None].expand(B, H, N, N).reshape(B * H, N, N), iters, warmup)
                rows.append({"tokens": N, "batch": B, "eager_ms": r(eager), "graph_replay_ms": r(replay), "torch_bf16_eager_ms": r(t_eager),
                             "torch_bf16_graph_replay_ms": t_replay and r(t_replay), "hip_over_torch_graph": t_replay and r(replay / t_replay), "rel_l2_vs_torch_bf16": agree,
                             "attn_span_ms": r(span_ms), "attn_dense_ms": r(dense_ms), "mask_expand_ms": r(expand_ms), "span_equals_dense_bitwise": same})
    return {"what": "GroundingDINO text side: spans + BERT-base + feat_map; host clock, median of 3 windows", "iters": iters, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.iters, a.warmup)), flush=True)
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
