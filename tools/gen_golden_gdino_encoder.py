"""Fixture generator for GroundingDINO's feature enhancer: tests/golden/gdino_enc_*.npz.

Runs on a development machine only: it loads the reference's own `models/GroundingDINO/transformer.py` BY FILE PATH (pass the reference checkout
with --reference or ANYEDIT_REFERENCE; nothing of it is copied into this tree) as a member of a synthetic package whose search path is that
directory, so that its relative imports (`.fuse_modules`, `.ms_deform_attn`, `.transformer_vanilla`, `.utils`) resolve to the reference's own
files, behind inert `sys.modules` stubs for the two foreign imports: `timm.models.layers.DropPath` (identity) and
`GroundingDINO.groundingdino.util.misc.inverse_sigmoid` (unused by the encoder).  The reference's deformable attention falls back to its pure
torch path on the CPU; no native extension is needed.  The tests read only the .npz files.  Chain of trust: the reference's TransformerEncoder
produces the stored outputs -> tests/gdino_enc_ref.py, a plain-torch restatement, is pinned to them at rel-L2 <= 1e-5 by the CPU suite -> the
GPU suite trusts the restatement at sizes no fixture could hold.

Two geometries with production head dims (fusion 256, text 64, deformable 32), which a d_model below 256 allows only through `pos_text`:
  a   d_model 64,  nhead 2, dim_feedforward 512,  2 layers, levels (9,7) (5,4) (3,2):          fusion 1 x 256, text 1 x 64, deformable 2 x 32
  b   d_model 128, nhead 4, dim_feedforward 1024, 1 layer,  levels (12,10) (6,5) (3,3) (2,2):  fusion 2 x 256, text 2 x 64, deformable 4 x 32
Both: bs 2; a padding mask on sample 1 (valid ratios below 1); 12 text tokens of which sample 1 has 7 valid; block-diagonal
text_self_attention_masks that differ per sample (with 2 text heads, geometry b pins the reference's `repeat` indexing);
pos_text = get_sine_pos_embed(position_ids[..., None], num_pos_feats=d_model, exchange_xy=False).

What the default init hides is re-drawn, every layer separately (`_get_clones` deep-copies one initialised layer): gamma_v / gamma_l from
U(0.5, 1.5) (default 1e-4 hides the fusion), LayerNorm weights from U(0.5, 1.5) and biases from N(0, 0.1^2), every Linear bias from N(0, 0.1^2)
except the sampling-offset bias (kept: the ring of directions), matrices from U(-a, a) with a = sqrt(3 / fan_in) (sampling_offsets half of that;
both it and attention_weights are zero by default).  Every weight is rounded to bf16 BEFORE the reference runs.

Files (none may pass the repository's 1 MiB limit), per geometry <g>:
  gdino_enc_<g>_w<i>.npz      w.<key>: a slice of the state dict as bf16 bits (int16); the slices are cut by size
  gdino_enc_<g>_io.npz        inputs (src, pos, spatial_shapes, level_start_index, valid_ratios, key_padding_mask, memory_text,
                              text_attention_mask, pos_text, text_self_attention_masks, position_ids), out / out_text, per layer and sub-block
                              tap.<layer>.<fusion|text|deform>.<v|l> (forward hooks), keys = the sorted state-dict key names
  gdino_enc_sine.npz          position_ids [2, 12] and get_sine_pos_embed(position_ids[..., None], 256, exchange_xy=False)
"""
import argparse
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOMS = {
    "a": dict(d_model=64, nhead=2, dff=512, num_layers=2, levels=[(9, 7), (5, 4), (3, 2)]),
    "b": dict(d_model=128, nhead=4, dff=1024, num_layers=1, levels=[(12, 10), (6, 5), (3, 3), (2, 2)]),
}
N_TEXT, N_TEXT_VALID_1 = 12, 7
W_FILE_BYTES = 900 * 1024


def load_reference(root):
    """The reference's transformer module, loaded by path inside a synthetic package, its two foreign imports stubbed."""
    layers = types.ModuleType("timm.models.layers")
    layers.DropPath = lambda *a, **k: torch.nn.Identity()
    misc = types.ModuleType("GroundingDINO.groundingdino.util.misc")
    misc.inverse_sigmoid = lambda x, eps=1e-3: torch.log(x.clamp(eps, 1 - eps) / (1 - x).clamp(eps, 1 - eps))
    stubs = {"timm": types.ModuleType("timm"), "timm.models": types.ModuleType("timm.models"), "timm.models.layers": layers,
             "GroundingDINO": types.ModuleType("GroundingDINO"), "GroundingDINO.groundingdino": types.ModuleType("GroundingDINO.groundingdino"),
             "GroundingDINO.groundingdino.util": types.ModuleType("GroundingDINO.groundingdino.util"), "GroundingDINO.groundingdino.util.misc": misc}
    for k, v in stubs.items():
        sys.modules.setdefault(k, v)
    d = os.path.join(root, "GroundingDINO", "groundingdino", "models", "GroundingDINO")
    pkg = types.ModuleType("reference_gdino")
    pkg.__path__ = [d]
    sys.modules["reference_gdino"] = pkg
    spec = importlib.util.spec_from_file_location("reference_gdino.transformer", os.path.join(d, "transformer.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_gdino.transformer"] = mod
    spec.loader.exec_module(mod)
    return mod


def redraw(m, g):
    norms = {k for k, mod in m.named_modules() if isinstance(mod, torch.nn.LayerNorm)}
    with torch.no_grad():
        for k, v in m.named_parameters():
            owner, leaf = k.rsplit(".", 1) if "." in k else ("", k)
            if leaf in ("gamma_v", "gamma_l"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif owner in norms:
                v.copy_(0.5 + torch.rand(v.shape, generator=g) if leaf == "weight" else 0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("sampling_offsets.bias"):
                pass
            elif v.dim() == 2:
                a = math.sqrt(3.0 / v.shape[1]) * (0.5 if k.endswith("sampling_offsets.weight") else 1.0)
                v.copy_((2 * torch.rand(v.shape, generator=g) - 1) * a)
            else:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            v.copy_(v.bfloat16().float())         # stored as bf16 bit patterns; the reference runs on these values


def make_inputs(geom, g):
    C, levels = geom["d_model"], geom["levels"]
    bs, n_img = 2, sum(h * w for h, w in levels)
    src = torch.randn(bs, n_img, C, generator=g)
    pos = 0.5 * torch.randn(bs, n_img, C, generator=g)
    kpm = torch.zeros(bs, n_img, dtype=torch.bool)
    ratios = torch.ones(bs, len(levels), 2)
    start, starts = 0, []
    for l, (H, W) in enumerate(levels):                 # sample 1: the right third and the bottom quarter of every level are padding
        starts.append(start)
        vh, vw = max(1, H - max(1, H // 4)), max(1, W - max(1, W // 3))
        m = torch.ones(H, W, dtype=torch.bool)
        m[:vh, :vw] = False
        kpm[1, start:start + H * W] = m.reshape(-1)
        ratios[1, l, 0], ratios[1, l, 1] = vw / W, vh / H
        start += H * W
    text = torch.randn(bs, N_TEXT, C, generator=g)
    tmask = torch.zeros(bs, N_TEXT, dtype=torch.bool)
    tmask[1, N_TEXT_VALID_1:] = True
    blocks = [[1, 3, 4, 3, 1], [1, 2, 3, 1, 1, 1, 1, 1, 1]]     # sub-sentence blocks per sample (sample 1: 7 valid tokens, then singletons)
    tsam = torch.zeros(bs, N_TEXT, N_TEXT, dtype=torch.bool)
    ids = torch.zeros(bs, N_TEXT, dtype=torch.long)
    for b, bl in enumerate(blocks):
        assert sum(bl) == N_TEXT
        s = 0
        for n in bl:
            tsam[b, s:s + n, s:s + n] = True
            ids[b, s:s + n] = torch.arange(n)
            s += n
    return dict(src=src, pos=pos, spatial_shapes=torch.tensor(levels, dtype=torch.long), level_start_index=torch.tensor(starts, dtype=torch.long),
                valid_ratios=ratios, key_padding_mask=kpm, memory_text=text, text_attention_mask=tmask, text_self_attention_masks=tsam, position_ids=ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    ref = load_reference(args.reference)
    utils = sys.modules["reference_gdino.utils"]
    import gdino_enc_ref as R
    rel = lambda a, b: float((a.detach().double() - b.detach().double()).norm() / b.detach().double().norm())
    bits = lambda v: v.detach().bfloat16().view(torch.int16).numpy()

    ids = torch.tensor([[0, 0, 1, 2, 0, 1, 2, 3, 4, 0, 1, 0], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]])
    emb = utils.get_sine_pos_embed(ids[..., None], num_pos_feats=256, exchange_xy=False)
    np.savez_compressed(os.path.join(OUT, "gdino_enc_sine.npz"), position_ids=ids.numpy(), embed=emb.numpy())

    for seed, (name, geom) in enumerate(GEOMS.items()):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(500 + seed)
        C, nhead, dff, nl = geom["d_model"], geom["nhead"], geom["dff"], geom["num_layers"]
        layer = ref.DeformableTransformerEncoderLayer(C, dff, 0.0, "relu", len(geom["levels"]), nhead, 4)
        text = ref.TransformerEncoderLayer(d_model=C, nhead=nhead // 2, dim_feedforward=dff // 2, dropout=0.1)
        fusion = ref.BiAttentionBlock(v_dim=C, l_dim=C, embed_dim=dff // 2, num_heads=nhead // 2, dropout=0.1, drop_path=0.0)
        m = ref.TransformerEncoder(layer, nl, d_model=C, text_enhance_layer=text, feature_fusion_layer=fusion)
        m.eval()
        redraw(m, g)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        files, cur, size = [], {}, 0
        for k in sorted(sd):
            n = sd[k].numel() * 2
            if cur and size + n > W_FILE_BYTES:
                files.append(cur)
                cur, size = {}, 0
            cur["w." + k] = bits(sd[k])
            size += n
        files.append(cur)
        for i, f in enumerate(files):
            np.savez_compressed(os.path.join(OUT, f"gdino_enc_{name}_w{i}.npz"), **f)

        inp = make_inputs(geom, g)
        inp["pos_text"] = utils.get_sine_pos_embed(inp["position_ids"][..., None], num_pos_feats=C, exchange_xy=False)
        taps = {}
        for i in range(nl):      # forward hooks: the streams after every sub-block
            m.fusion_layers[i].register_forward_hook(lambda mod, a, out, i=i: taps.update({f"tap.{i}.fusion.v": out[0].detach().clone(), f"tap.{i}.fusion.l": out[1].detach().clone()}))
            m.text_layers[i].register_forward_hook(lambda mod, a, out, i=i: taps.update({f"tap.{i}.text.l": out.detach().transpose(0, 1).clone()}))
            m.layers[i].register_forward_hook(lambda mod, a, out, i=i: taps.update({f"tap.{i}.deform.v": out.detach().clone()}))
        with torch.no_grad():
            out, out_text = m(src=inp["src"], pos=inp["pos"], spatial_shapes=inp["spatial_shapes"], level_start_index=inp["level_start_index"],
                              valid_ratios=inp["valid_ratios"], key_padding_mask=inp["key_padding_mask"], memory_text=inp["memory_text"],
                              text_attention_mask=inp["text_attention_mask"], pos_text=inp["pos_text"],
                              text_self_attention_masks=inp["text_self_attention_masks"], position_ids=None)
        assert torch.isfinite(out).all() and torch.isfinite(out_text).all()
        o = {k: v.numpy() for k, v in inp.items()}
        o.update({k: v.numpy() for k, v in taps.items()})
        o["out"], o["out_text"] = out.numpy(), out_text.numpy()
        o["keys"] = np.array(sorted(sd))
        np.savez_compressed(os.path.join(OUT, f"gdino_enc_{name}_io.npz"), **o)

        cfg = dict(num_layers=nl, nhead=nhead, enc_n_points=4)
        mine = R.encoder_forward(sd, cfg, inp["src"], inp["pos"], geom["levels"], inp["valid_ratios"], inp["key_padding_mask"], inp["memory_text"],
                                 inp["text_attention_mask"], pos_text=inp["pos_text"], text_self_attention_masks=inp["text_self_attention_masks"])
        print(f"{name}: restatement vs reference rel-L2: image {rel(mine[0], out):.2e} text {rel(mine[1], out_text):.2e}")
    print("sine: restatement vs reference %.2e" % rel(R.sine_pos_embed(ids[..., None], 256, exchange_xy=False), emb))
    for f in sorted(os.listdir(OUT)):
        if f.startswith("gdino_enc"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
