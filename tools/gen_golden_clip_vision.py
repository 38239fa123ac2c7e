"""Fixture generator for the CLIP vision tower: tests/golden/clip_vision_tiny*.npz.

Runs on a development machine only (needs `transformers` on the CPU, offline); the tests read the fixtures and do not need it.  Chain of
trust: transformers' CLIPVisionModelWithProjection produces the stored outputs -> tests/clip_vision_ref.py, a plain-torch restatement, is
pinned to them at rel-L2 <= 1e-5 by the CPU suite -> the GPU suite trusts the restatement at sizes no fixture could hold.

Two geometries, so that both head dims of the real towers and both activations are pinned (2 layers, 2 heads each):
  quick_gelu   width 128 = 2 x 64, patch 14, image 70 (25 + 1 tokens; 588 real patch columns, padded to 640 on the HIP path),
               intermediate 256, projection 96
  gelu         width 160 = 2 x 80, patch 16, image 48 (9 + 1 tokens), intermediate 128, projection 64
The default init is rescaled as tools/gen_golden_clip.py does (2-D matrix weights x 3, biases N(0, 0.1)) so the logits are not
degenerate; every weight is rounded to bf16 BEFORE transformers runs, so the stored bit patterns are what it computed on.

Files (one npz cannot hold everything under the repository's 1 MiB-per-file limit), per geometry <act>:
  clip_vision_tiny_<act>.npz       w.<key> weights (bf16 bits as int16, Hugging Face keys: vision_model.*, visual_projection.weight)
  clip_vision_tiny_<act>_out.npz   pixels_u8 [3, 3, S, S] raw pixels (image 2 all zero), pixel_values [3, 3, S, S] fp32: images 0 and 1 the
                                   CLIP-normalised pixels_u8, image 2 ALL ZERO (train.py:682: the reference image may be a zero tensor);
                                   image_embeds, last_hidden_state, pooler_output, hidden_states.<i> of transformers on pixel_values
"""
import os
os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOMS = {
    "quick_gelu": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=70,
                       projection_dim=96, hidden_act="quick_gelu", layer_norm_eps=1e-5),
    "gelu": dict(hidden_size=160, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=16, image_size=48,
                 projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5),
}


def hf_keys(sd):
    """transformers versions that drop the `vision_model.` level from CLIPVisionModelWithProjection.state_dict(): added back here."""
    if any(k.startswith("vision_model.") for k in sd):
        return dict(sd)
    return {(k if k.startswith("visual_projection.") else "vision_model." + k): v for k, v in sd.items()}


def main():
    from transformers import CLIPVisionModelWithProjection, CLIPVisionConfig
    import clip_vision_ref
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    for seed, (act, geom) in enumerate(GEOMS.items()):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(100 + seed)
        m = CLIPVisionModelWithProjection(CLIPVisionConfig(**geom)).eval()
        with torch.no_grad():
            for k, v in m.named_parameters():
                if v.ndim == 2 and "embedding" not in k:
                    v.mul_(3.0)
                if k.endswith("bias"):
                    v.copy_(torch.randn(v.shape, generator=g) * 0.1)
                v.copy_(v.bfloat16().float())     # stored as bf16 bit patterns; transformers runs on these values
        sd = {k: v.detach().clone() for k, v in hf_keys(m.state_dict()).items() if not k.endswith("position_ids")}
        S = geom["image_size"]
        u8 = torch.randint(0, 256, (3, 3, S, S), generator=g, dtype=torch.uint8)
        u8[2] = 0
        px = clip_vision_ref.normalize_u8(u8)
        px[2] = 0.0
        with torch.no_grad():
            out = m(pixel_values=px, output_hidden_states=True)
        o = {"pixels_u8": u8.numpy(), "pixel_values": px.numpy(), "image_embeds": out.image_embeds.numpy(),
             "last_hidden_state": out.last_hidden_state.numpy()}
        # the pooled row (post_layernorm of the class token) is what visual_projection reads
        with torch.no_grad():
            pooled = m.vision_model.post_layernorm(out.last_hidden_state[:, 0])
            assert rel(m.visual_projection(pooled), out.image_embeds) < 1e-6
        o["pooler_output"] = pooled.numpy()
        for i, h in enumerate(out.hidden_states):
            o[f"hidden_states.{i}"] = h.numpy()
        assert torch.equal(out.hidden_states[-1], out.last_hidden_state), "last_hidden_state carries no final norm"
        mine = clip_vision_ref.clip_vision_forward(sd, px, geom["num_attention_heads"], act=act, eps=geom["layer_norm_eps"])
        print(act, "embeds std", float(out.image_embeds.std()), "restatement vs transformers rel-L2: embeds", rel(mine["image_embeds"], out.image_embeds),
              "hidden", [rel(a, b) for a, b in zip(mine["hidden_states"], out.hidden_states)])
        np.savez_compressed(os.path.join(OUT, f"clip_vision_tiny_{act}.npz"), **{"w." + k: v.bfloat16().view(torch.int16).numpy() for k, v in sd.items()})
        np.savez_compressed(os.path.join(OUT, f"clip_vision_tiny_{act}_out.npz"), **o)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("clip_vision_tiny"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
