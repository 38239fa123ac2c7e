"""Fixture generator for the CLIP text tower: tests/golden/clip_text_tiny*.npz.

Runs on a development machine only (needs `transformers` on the CPU, offline, and the reference checkout for cldm/hack.py); the tests read
the fixtures and need neither.  Chain of trust: transformers' CLIPTextModel (and the reference's own `_hacked_clip_forward`) produce the
stored outputs -> tests/clip_ref.py, a plain-torch restatement, is pinned to them at rel-L2 <= 1e-5 by the CPU suite -> the GPU suite trusts
the restatement at sizes no fixture could hold.

Geometry: vocab 256, width 128 = 2 heads x 64, 2 layers, intermediate 512, 77 positions; eos = pad = 255, bos = 254.  The EOS id is the
largest id on purpose: the reference-era rule for the pooled row (argmax of the ids) and the current one (first EOS) then pick the same
position — asserted below.  The default init is rescaled (matrix weights x 3, biases N(0, 0.1)) so the logits are not degenerate and the
causal mask matters; every weight is rounded to bf16 BEFORE transformers runs, so the stored bit patterns are what it computed on.

Files (one npz cannot hold everything under the repository's 1 MiB-per-file limit):
  clip_text_tiny.npz             w.<key> weights (bf16 bits as int16, keys as in SD-1.5 checkpoints below cond_stage_model.), input_ids [4, 77]
                                 (EOS at 9, 40, 76 — a row with no padding — and 1, the empty prompt), raw.<n> token lists, framed [4, 3, 77]
  clip_text_tiny_quick_gelu.npz  last_hidden_state, hidden_states.<i>, pooler_output for hidden_act = quick_gelu
  clip_text_tiny_gelu.npz        the same for an erf-GELU copy of the config (same weights)
  clip_text_tiny_hack<k>.npz     the reference's _hacked_clip_forward for clip_skip k = 0, 2 on raw token lists of lengths 5, 75, 76, 200
"""
import os
os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"
import sys
import types
import importlib.util

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOM = dict(vocab_size=256, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
            eos_token_id=255, pad_token_id=255, bos_token_id=254)
PREFIX = "transformer.text_model."   # transformers >= 5 dropped the text_model level from CLIPTextModel.state_dict(): added back here


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference_hack():
    """cldm/hack.py by file path, with inert stand-ins for the two ldm modules it imports at the top (their own imports — open_clip, kornia —
    are not needed by _hacked_clip_forward)."""
    class FrozenCLIPEmbedder:
        pass
    ldm = _mod("ldm"); mods = _mod("ldm.modules"); enc = _mod("ldm.modules.encoders")
    em = _mod("ldm.modules.encoders.modules", FrozenCLIPEmbedder=FrozenCLIPEmbedder)
    at = _mod("ldm.modules.attention", default=lambda v, d: v if v is not None else d, CrossAttention=type("CrossAttention", (), {}))
    ldm.modules, mods.encoders, mods.attention, enc.modules = mods, enc, at, em
    spec = importlib.util.spec_from_file_location("ref_cldm_hack", os.path.join(REF, "AnyEdit_Collection", "other_modules", "cldm", "hack.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class StubTokenizer:
    pad_token_id, eos_token_id, bos_token_id = GEOM["pad_token_id"], GEOM["eos_token_id"], GEOM["bos_token_id"]

    def __init__(self, raw):
        self.raw = raw

    def __call__(self, text, truncation=False, add_special_tokens=False, **_):
        assert not truncation and not add_special_tokens
        return {"input_ids": [list(r) for r in self.raw]}


def main():
    from transformers import CLIPTextModel, CLIPTextConfig
    import clip_ref
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    models = {}
    for act in ("quick_gelu", "gelu"):
        models[act] = CLIPTextModel(CLIPTextConfig(**GEOM, hidden_act=act)).eval()
    m = models["quick_gelu"]
    with torch.no_grad():
        for k, v in m.named_parameters():
            if v.ndim == 2 and "embedding" not in k:
                v.mul_(3.0)
            if k.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.1)
            v.copy_(v.bfloat16().float())     # stored as bf16 bit patterns; transformers runs on these values
    models["gelu"].load_state_dict(m.state_dict())
    sd = {PREFIX + k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith("position_ids")}
    V, EOS, BOS = GEOM["vocab_size"], GEOM["eos_token_id"], GEOM["bos_token_id"]

    ids = torch.randint(0, V - 2, (4, 77), generator=g)
    ids[:, 0] = BOS
    for b, n in enumerate((9, 40, 76, 1)):
        ids[b, n:] = EOS
    assert torch.equal(ids.argmax(-1), (ids == EOS).int().argmax(-1)), "the legacy (argmax) and current (first EOS) pooled rules must agree"

    arrs = {"w." + k: v.bfloat16().view(torch.int16).numpy() for k, v in sd.items()}
    arrs["input_ids"] = ids.numpy().astype(np.int64)
    raw = [torch.randint(0, V - 2, (n,), generator=g).tolist() for n in (5, 75, 76, 200)]
    for i, r in enumerate(raw):
        arrs[f"raw.{i}"] = np.asarray(r, dtype=np.int64)

    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    for act, mod in models.items():
        with torch.no_grad():
            out = mod(input_ids=ids, output_hidden_states=True)
        o = {"last_hidden_state": out.last_hidden_state.numpy(), "pooler_output": out.pooler_output.numpy()}
        for i, h in enumerate(out.hidden_states):
            o[f"hidden_states.{i}"] = h.numpy()
        mine = clip_ref.clip_text_forward(sd, ids, GEOM["num_attention_heads"], act=act, eos_token_id=EOS)
        print(act, "std", float(out.last_hidden_state.std()), "restatement vs transformers rel-L2: last", rel(mine["last_hidden_state"], out.last_hidden_state),
              "pooled", rel(mine["pooler_output"], out.pooler_output), "hidden", [rel(a, b) for a, b in zip(mine["hidden_states"], out.hidden_states)])
        np.savez_compressed(os.path.join(OUT, f"clip_text_tiny_{act}.npz"), **o)

    hack = load_reference_hack()
    framed = None
    for skip in (0, 2):
        tr = types.SimpleNamespace(text_model=types.SimpleNamespace(final_layer_norm=m.final_layer_norm))
        shim = type("Shim", (), {"__call__": lambda self, **kw: m(**kw), "text_model": tr.text_model})()
        me = types.SimpleNamespace(tokenizer=StubTokenizer(raw), transformer=shim, clip_skip=skip, device="cpu")
        seen = {}
        orig = m.forward
        def spy(*a, **kw):
            seen["ids"] = kw["input_ids"].clone()
            return orig(*a, **kw)
        m.forward = spy
        with torch.no_grad():
            z = hack._hacked_clip_forward(me, ["a", "b", "c", "d"])
        m.forward = orig
        framed = seen["ids"].reshape(4, 3, 77).long()
        mine = clip_ref.hacked_forward(sd, framed, GEOM["num_attention_heads"], clip_skip=skip)
        print("hack clip_skip", skip, tuple(z.shape), "restatement rel-L2", rel(mine, z))
        np.savez_compressed(os.path.join(OUT, f"clip_text_tiny_hack{skip}.npz"), z=z.numpy())
    arrs["framed"] = framed.numpy().astype(np.int64)
    np.savez_compressed(os.path.join(OUT, "clip_text_tiny.npz"), **arrs)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("clip_text_tiny"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
