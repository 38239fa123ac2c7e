"""Fixture generator for the device code of GroundingDINO's query selection and decoder: tests/golden/gdino_dec_geom.npz.

Runs on a development machine only.  It loads the reference's own `models/GroundingDINO/transformer.py` by file path with the stub technique of
tools/gen_golden_gdino_encoder.py (its `load_reference`), so `gen_encoder_output_proposals`, `gen_sineembed_for_position` and `ContrastiveEmbed`
are the reference's own `utils.py`; nothing of it is copied into this tree.  The tests read only the .npz file.

gdino_dec_geom.npz — functions only, no weights:
  levels (1,1) (3,5) (4,3) (2,2), bs 3: sample 0 unpadded, sample 1 with valid_W < W and valid_H < H on every level that has room (the (3,5)
  level keeps 3 of 5 columns: a non-square level with valid_W < W), sample 2 padded everywhere except one cell per level.
  padding_mask, spatial_shapes, proposals (gen_encoder_output_proposals's second output), memory_kept (which rows of an all-ones memory its first
  output keeps), boxes [2, 6, 4] with exact 0 / 0.5 / 1 entries and sineembed = gen_sineembed_for_position(boxes),
  ce_x / ce_y / ce_mask and ce_out = ContrastiveEmbed(max_text_len=16)(x, {...}).

gdino_dec_w<i>.npz / gdino_dec_io.npz — the tower: the reference's Transformer at d_model 256, nhead 8, dim_feedforward 64, no encoder layers, 2 decoder
  layers, levels (9,7) (5,4) (3,2), bs 2, 20 queries, 12 text tokens of which sample 1 uses 7, a padding mask on sample 1 (the last column of the finest level: 9 rows that tie), two_stage_type "standard",
  embed_init_tgt, use_text_cross_attention; heads wired as groundingdino.py:163-197 wires them for the SwinB config (decoder box head shared,
  enc_out_bbox_embed a separate copy).  What the default init hides is re-drawn (zero last box layer, zero offset / weight matrices, LayerNorms,
  biases), every weight rounded to bf16 BEFORE the reference runs and stored as bf16 bits in slices under the 1 MiB limit (w.<key>).  io: src.l /
  mask.l / pos.l, text, token_mask, topk_logits (every row), topk_proposals, hs, references, hs_enc, ref_enc, init_box_proposal, per layer
  dec.<l>.output / reference_points / query_sine_embed (forward hooks), pred_logits.<l> / pred_boxes.<l> (groundingdino.py:317-335 restated from
  the reference's own MLP / ContrastiveEmbed objects), keys; the same with the prefix no. for a two_stage_type "no" model that reuses the weights
  (+ refpoint_embed.weight).  Seeds are tried until the 20th and 21st reference score of each sample differ by more than 1e-3 and a selected row of
  sample 1 is a padded or invalid row.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LEVELS = [(1, 1), (3, 5), (4, 3), (2, 2)]


def padding_mask():
    n = sum(h * w for h, w in LEVELS)
    m = torch.zeros(3, n, dtype=torch.bool)
    s = 0
    for H, W in LEVELS:
        a = torch.ones(H, W, dtype=torch.bool)
        a[:max(1, H - 1), :max(1, W - 2)] = False
        m[1, s:s + H * W] = a.reshape(-1)
        b = torch.ones(H, W, dtype=torch.bool)
        b[0, 0] = False
        m[2, s:s + H * W] = b.reshape(-1)
        s += H * W
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    from gen_golden_gdino_encoder import load_reference
    load_reference(args.reference)
    utils = sys.modules["reference_gdino.utils"]
    import gdino_dec_ref as R
    g = torch.Generator().manual_seed(77)

    m = padding_mask()
    shapes = torch.tensor(LEVELS, dtype=torch.long)
    mem, prop = utils.gen_encoder_output_proposals(torch.ones(3, m.shape[1], 2), m, shapes)
    boxes = torch.rand(2, 6, 4, generator=g)
    boxes[0, 0] = torch.tensor([0.0, 1.0, 0.5, 0.0])
    boxes[1, 5] = torch.tensor([1.0, 0.0, 1.0, 0.5])
    sine = utils.gen_sineembed_for_position(boxes)
    x, y = torch.randn(2, 5, 32, generator=g), torch.randn(2, 12, 32, generator=g)
    tm = torch.ones(2, 12, dtype=torch.bool)
    tm[1, 7:] = False
    ce = utils.ContrastiveEmbed(max_text_len=16)(x, {"encoded_text": y, "text_token_mask": tm})
    np.savez_compressed(os.path.join(OUT, "gdino_dec_geom.npz"), padding_mask=m.numpy(), spatial_shapes=shapes.numpy(), proposals=prop.numpy(),
                        memory_kept=(mem[..., 0] != 0).numpy(), boxes=boxes.numpy(), sineembed=sine.numpy(), ce_x=x.numpy(), ce_y=y.numpy(),
                        ce_mask=tm.numpy(), ce_out=ce.numpy())

    mine, keep = R.encoder_output_proposals(m, LEVELS)
    fin = torch.isfinite(prop)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    print("proposals: inf pattern equal", bool((torch.isfinite(mine) == fin).all()), " kept rows equal", bool((keep == (mem[..., 0] != 0)).all()),
          " finite rel-L2 %.2e" % rel(mine[fin], prop[fin]), " finite rows", int(keep.sum()), "of", keep.numel())
    print("sineembed rel-L2 %.2e" % rel(R.query_sine_embed(boxes), sine), " contrastive equal", bool((R.contrastive(x, y, tm, 16) == ce).all()))
    print("gdino_dec_geom.npz", os.path.getsize(os.path.join(OUT, "gdino_dec_geom.npz")))
    tower(args)


def redraw(m, g):
    import math
    norms = {k for k, mod in m.named_modules() if isinstance(mod, torch.nn.LayerNorm)}
    with torch.no_grad():
        for k, v in m.named_parameters():
            owner, leaf = k.rsplit(".", 1) if "." in k else ("", k)
            if owner in norms:
                v.copy_(0.5 + torch.rand(v.shape, generator=g) if leaf == "weight" else 0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("sampling_offsets.bias"):
                pass
            elif "embed.weight" in k and "bbox" not in k:          # tgt_embed / refpoint_embed
                v.copy_(torch.randn(v.shape, generator=g))
            elif v.dim() == 2:
                a = math.sqrt(3.0 / v.shape[1]) * (0.5 if k.endswith("sampling_offsets.weight") else 1.0)
                v.copy_((2 * torch.rand(v.shape, generator=g) - 1) * a)
            else:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            v.copy_(v.bfloat16().float())


def build(ref, utils, R, two_stage):
    import copy
    G = R.GEOM
    m = ref.Transformer(d_model=G["d_model"], nhead=G["nhead"], num_queries=G["num_queries"], num_encoder_layers=0, num_decoder_layers=G["num_decoder_layers"],
                        dim_feedforward=G["dff"], dropout=0.0, return_intermediate_dec=True, num_feature_levels=len(G["levels"]), learnable_tgt_init=True,
                        two_stage_type=two_stage, embed_init_tgt=True, use_text_cross_attention=True)
    box = utils.MLP(256, 256, 4, 3)
    m.decoder.bbox_embed = torch.nn.ModuleList([box] * G["num_decoder_layers"])
    m.decoder.class_embed = torch.nn.ModuleList([utils.ContrastiveEmbed()] * G["num_decoder_layers"])
    if two_stage == "standard":
        m.enc_out_bbox_embed, m.enc_out_class_embed = copy.deepcopy(box), utils.ContrastiveEmbed()
    return m.eval()


def run(m, inp, utils, misc, prefix=""):
    G_L = len(inp["srcs"])
    taps = {}
    for i, layer in enumerate(m.decoder.layers):
        def hook(mod, args, kwargs, out, i=i):
            taps[f"{prefix}dec.{i}.output"] = out.detach().transpose(0, 1).clone()
            taps[f"{prefix}dec.{i}.query_sine_embed"] = kwargs["tgt_query_sine_embed"].detach().transpose(0, 1).clone()
        layer.register_forward_hook(hook, with_kwargs=True)
    td = {"encoded_text": inp["text"].clone(), "text_token_mask": inp["token_mask"], "position_ids": None, "text_self_attention_masks": None}
    with torch.no_grad():
        hs, refs, hs_enc, ref_enc, ibp = m(inp["srcs"], inp["masks"], None, inp["poss"], None, None, td)
        o = {prefix + "hs": torch.stack(hs), prefix + "references": torch.stack(refs), prefix + "init_box_proposal": ibp}
        for l in range(len(hs)):
            o[f"{prefix}dec.{l}.reference_points"] = refs[l]
            o[f"{prefix}pred_boxes.{l}"] = (m.decoder.bbox_embed[l](hs[l]) + misc.inverse_sigmoid(refs[l])).sigmoid()
            o[f"{prefix}pred_logits.{l}"] = m.decoder.class_embed[l](hs[l], td)
        if hs_enc is not None:
            o[prefix + "hs_enc"], o[prefix + "ref_enc"] = hs_enc, ref_enc
    o.update(taps)
    return o


def tower(args):
    from gen_golden_gdino_encoder import load_reference
    ref = load_reference(args.reference)
    utils = sys.modules["reference_gdino.utils"]
    misc = sys.modules["GroundingDINO.groundingdino.util.misc"]

    # util/misc.py is a foreign import of the reference's transformer.py (the encoder generator stubs it); the decoder and the heads call its
    # inverse_sigmoid, so the real file is loaded by path here, behind an inert stub for its `torchvision` import, and its function put in place
    import importlib.util
    import types
    sys.modules.setdefault("torchvision", types.SimpleNamespace(__version__="0.15.0"))
    spec = importlib.util.spec_from_file_location("reference_gdino_misc", os.path.join(args.reference, "GroundingDINO", "groundingdino", "util", "misc.py"))
    real = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(real)
    misc.inverse_sigmoid = ref.inverse_sigmoid = real.inverse_sigmoid
    import gdino_dec_ref as R
    G = R.GEOM
    for seed in range(400):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(900 + seed)
        m = build(ref, utils, R, "standard")
        redraw(m, g)
        srcs, masks, poss = [], [], []
        for H, W in G["levels"]:
            srcs.append(torch.randn(G["bs"], 256, H, W, generator=g))
            poss.append(0.5 * torch.randn(G["bs"], 256, H, W, generator=g))
            mk = torch.zeros(G["bs"], H, W, dtype=torch.bool)
            if (H, W) == G["levels"][0]:          # sample 1: the last column of the finest level is padding (a seventh of the width rounds to
                mk[1, :, W - 1:] = True           # nothing at the coarser levels).  Few masked rows ON PURPOSE: they all tie, so a selection with a
                                                  # gap behind its last slot can hold masked rows only if it holds all of them
            masks.append(mk)
        text = torch.randn(G["bs"], G["n_text"], 256, generator=g)
        tm = torch.ones(G["bs"], G["n_text"], dtype=torch.bool)
        tm[1, G["n_text_used_1"]:] = False
        inp = dict(srcs=srcs, masks=masks, poss=poss, text=text, token_mask=tm)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        cfg = dict(G)
        mine = R.transformer_forward(sd, cfg, srcs, masks, text, tm)
        score, idx = mine["topk_logits"], mine["topk_proposals"]
        srt = torch.sort(score, 1, descending=True)[0]
        gap = float((srt[:, G["num_queries"] - 1] - srt[:, G["num_queries"]]).min())
        _, keep = R.encoder_output_proposals(torch.cat([k.flatten(1) for k in masks], 1), G["levels"])
        bad_selected = int((~keep[1][idx[1]]).sum())
        if gap > 1e-3 and bad_selected >= 1:
            break
    else:
        raise SystemExit("no seed met the two conditions")
    print(f"seed {seed}: gap between the 20th and 21st score {gap:.3e}; {bad_selected} selected rows of sample 1 are padded or invalid")
    o = run(m, inp, utils, misc)
    o["topk_logits"], o["topk_proposals"] = score, idx
    assert torch.equal(torch.topk(score, G["num_queries"], dim=1)[1], idx)
    m2 = build(ref, utils, R, "no")
    g2 = torch.Generator().manual_seed(5000 + seed)
    rp = (torch.randn(G["num_queries"], 4, generator=g2)).bfloat16().float()
    sd2 = {k: v for k, v in sd.items() if not k.startswith(("enc_out", "enc_output"))}
    sd2["refpoint_embed.weight"] = rp
    m2.load_state_dict(sd2, strict=True)
    o.update(run(m2, inp, utils, misc, prefix="no."))
    sd["refpoint_embed.weight"] = rp
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    mine2 = R.transformer_forward(sd, cfg, srcs, masks, text, tm, two_stage="no")
    worst = max([rel(mine[k], o[k]) for k in o if not k.startswith("no.") and k in mine and o[k].dtype.is_floating_point and torch.isfinite(o[k]).all()]
                + [rel(mine2[k[3:]], o[k]) for k in o if k.startswith("no.") and torch.isfinite(o[k]).all()])
    print(f"restatement vs reference, worst rel-L2 over {len(o)} tensors: {worst:.2e}")
    bits = lambda v: v.detach().bfloat16().view(torch.int16).numpy()
    files, cur, size = [], {}, 0
    for k in sorted(sd):
        n = sd[k].numel() * 2
        if cur and size + n > 900 * 1024:
            files.append(cur)
            cur, size = {}, 0
        cur["w." + k] = bits(sd[k])
        size += n
    files.append(cur)
    for i, f in enumerate(files):
        np.savez_compressed(os.path.join(OUT, f"gdino_dec_w{i}.npz"), **f)
    io = {k: v.numpy() for k, v in o.items()}
    for l in range(len(srcs)):
        io[f"src.{l}"], io[f"mask.{l}"], io[f"pos.{l}"] = srcs[l].numpy(), masks[l].numpy(), poss[l].numpy()
    io["text"], io["token_mask"] = text.numpy(), tm.numpy()
    io["keys"] = np.array(sorted(k for k in sd if k != "refpoint_embed.weight"))
    io["no.keys"] = np.array(sorted(sd2))
    np.savez_compressed(os.path.join(OUT, "gdino_dec_io.npz"), **io)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("gdino_dec"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
