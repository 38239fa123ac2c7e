"""Time of one CLIP text encode (FrozenCLIPEmbedder.encode_ids, ViT-L/14 text geometry, seeded weights) at B = 1 / 3 / 4 / 12 prompts of 77
tokens: eager (launch-per-op from Python) and as a replayed graph.

    python tools/encode_prompt.py [--iters 200] [--warmup 20] [--batches 1 3 4 12] [--out FILE]

Each figure is a host clock around `iters` encodes that ends in a device synchronise (the clock is read after the synchronise), after
`warmup` untimed encodes of the same shape; the window is repeated 3 times and the median is reported with the spread.  If `transformers`
is importable its bf16 CLIPTextModel on the same ids is timed the same way as a yardstick; otherwise the line says it is absent.
Prints one JSON line per batch size.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HF_HUB_OFFLINE", "1")


def timed(fn, iters, warmup, windows=3):
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


def hf_yardstick(sd, cfg, ids, iters, warmup):
    try:
        from transformers import CLIPTextModel, CLIPTextConfig
    except Exception as e:  # noqa: BLE001
        return None, f"transformers not importable ({type(e).__name__})"
    keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings", "hidden_act",
            "layer_norm_eps", "eos_token_id", "bos_token_id", "pad_token_id")
    m = CLIPTextModel(CLIPTextConfig(**{k: cfg[k] for k in keys})).eval()
    own = set(m.state_dict())
    strip = "transformer.text_model." if "embeddings.token_embedding.weight" in own else "transformer."
    m.load_state_dict({k[len(strip):]: v for k, v in sd.items()})
    m = m.to("cuda", torch.bfloat16)
    with torch.no_grad():
        return timed(lambda: m(input_ids=ids).last_hidden_state, iters, warmup), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 3, 4, 12])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import clip_ref
    from anyedit_amd import _lib
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder, CLIP_VIT_L_TEXT as cfg
    sd = clip_ref.seeded_state_dict(cfg, seed=0)
    with torch.device("meta"):
        te = FrozenCLIPEmbedder()
    te.load_state_dict(sd, assign=True)
    te = te.to("cuda")
    lines = [json.dumps({"device": _lib.device_arch(), "iters": a.iters, "warmup": a.warmup, "geometry": "ViT-L/14 text, 77 tokens"})]
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for B in a.batches:
            ids = torch.randint(0, cfg["vocab_size"] - 2, (B, 77), generator=gen)
            ids[:, 0] = cfg["bos_token_id"]
            ids[:, 20:] = cfg["eos_token_id"]
            dev_ids = ids.to("cuda")
            eager = timed(lambda: te.encode_ids(dev_ids), a.iters, a.warmup)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = te.encode_ids(dev_ids)
            replay = timed(graph.replay, a.iters, a.warmup)
            assert torch.isfinite(out).all()
            hf, why = hf_yardstick(sd, cfg, dev_ids, a.iters, a.warmup)
            r = {"B": B, "eager_ms": round(eager[0], 4), "eager_min_max_ms": [round(eager[1], 4), round(eager[2], 4)],
                 "graph_replay_ms": round(replay[0], 4), "graph_min_max_ms": [round(replay[1], 4), round(replay[2], 4)],
                 "transformers_bf16_ms": None if hf is None else round(hf[0], 4)}
            if why:
                r["transformers"] = why
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
