"""Restatement in fp32 torch (CPU) of GroundingDINO.forward behind the tokenizer (groundingdino.py:233-335) from the pinned restatements of its parts:
swin_ref (the tower), bert_ref (sub-sentence rule, BERT, feat_map), gdino_neck_ref (input_proj, level masks, sine embedding) and gdino_dec_ref
(Transformer.forward + the heads).  `store=round_bf16` makes the bf16-storage control: every activation the HIP path stores in bf16 is rounded at
that point (the parts' own `# bf16:` marks, plus src_flatten after the GroupNorm and pos_flatten after the sine).

Also the tiny detector the CPU and GPU suites share: the geometries of the fixtures swin_tiny_a (stages 1 and 2 out), bert_tiny_a and the tiny
transformer of gdino_dec_w* (three levels: two backbone levels and one stride-2 level; no encoder layers, so no level embedding), seeded weights
rounded to bf16 for the towers and input_proj, the transformer's golden weights.
"""
import torch

import bert_ref as BR
import gdino_dec_ref as DR
import gdino_neck_ref as NR
import swin_ref as SR

SWIN = dict(embed_dim=32, depths=[2, 2, 2], num_heads=[1, 2, 4], window_size=7, out_indices=(1, 2))
TEMPERATURE = (20, 20)
SIZES = ((50, 38), (40, 40))           # two images, padded to 50 x 40: a real padding mask, ragged stage sizes (7x5, 4x3) and a 2x2 stride-2 level
CAPTIONS = ["cat . red dog .", "a chair ."]


class StandInTokenizer:
    """The Hugging Face call signature over a whitespace vocabulary: [CLS] words [SEP], padded to the longest with 0; a single string gives
    unpadded lists, as `tokenizer(caption)` of tools/tool.py:137 does; `decode` joins the words."""
    VOCAB = {"[PAD]": 0, "[CLS]": 1, "[SEP]": 2, ".": 3, "?": 4, "cat": 10, "dog": 11, "a": 12, "red": 13, "chair": 14}

    def convert_tokens_to_ids(self, tokens):
        return [self.VOCAB[t] for t in tokens]

    def _ids(self, caption):
        return [1] + [self.VOCAB[w] for w in caption.split()] + [2]

    def __call__(self, captions, padding=False, return_tensors=None):
        if isinstance(captions, str):
            ids = self._ids(captions)
            return {"input_ids": ids, "attention_mask": [1] * len(ids), "token_type_ids": [0] * len(ids)}
        assert padding == "longest" and return_tensors == "pt"
        rows = [self._ids(c) for c in captions]
        n = max(len(r) for r in rows)
        ids = torch.tensor([r + [0] * (n - len(r)) for r in rows])
        return {"input_ids": ids, "attention_mask": (ids != 0).long(), "token_type_ids": torch.zeros_like(ids)}

    def decode(self, token_ids):
        words = {v: k for k, v in self.VOCAB.items()}
        return " ".join(words[int(t)] for t in token_ids)


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def model_forward(sd, px, mask, ids, token_mask, special_ids, bert_heads, store=None, topk_proposals=None, two_stage="standard"):
    """sd: the detector's state dict (the reference's names); px fp32 [B, 3, H, W]; mask bool [B, H, W] (True = padding); ids / token_mask [B, T]
    (the tokenizer's input_ids and attention_mask).  Returns pred_logits / pred_boxes of the last decoder layer, src_flatten, pos_flatten,
    mask_flatten, topk_logits, topk_proposals."""
    bf = store is not None
    st = store if bf else (lambda t: t)
    sw = SR.swin_forward(_sub(sd, "backbone.0."), px, SWIN, bf16_storage=bf)
    spans, position_ids = BR.text_spans(ids, special_ids)
    bo = BR.bert_forward(sd, ids, bert_heads, allowed=BR.spans_to_mask(spans), position_ids=position_ids, bf16_storage=bf, prefix="bert.")
    text = BR.feat_map(sd, bo["last_hidden_state"], bf16_storage=bf)
    srcs = []
    n_proj = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("input_proj."))
    for l in range(n_proj):
        p = f"input_proj.{l}."
        if l < len(sw["outs"]):
            x, stride = sw["outs"][l], 1
        else:
            x, stride = (sw["outs"][-1] if l == len(sw["outs"]) else srcs[-1]), 2                  # groundingdino.py:300-304
        srcs.append(st(NR.input_proj(x, sd[p + "0.weight"], sd[p + "0.bias"], sd[p + "1.weight"], sd[p + "1.bias"], stride)))
    masks = [NR.level_mask(mask, *s.shape[-2:]) for s in srcs]
    poss = [st(NR.position_sine(m, 128, TEMPERATURE[0], TEMPERATURE[1], torch.float32)) for m in masks]
    tsd = _sub(sd, "transformer.")
    cfg = dict(DR.GEOM, levels=[tuple(s.shape[-2:]) for s in srcs])
    out = DR.transformer_forward(tsd, cfg, srcs, masks, text, token_mask.bool(), two_stage=two_stage, store=store, topk_proposals=topk_proposals)
    last = cfg["num_decoder_layers"] - 1
    flat = lambda ts: torch.cat([t.flatten(2).transpose(1, 2) for t in ts], 1)
    return dict(pred_logits=out[f"pred_logits.{last}"], pred_boxes=out[f"pred_boxes.{last}"], src_flatten=flat(srcs),
                pos_flatten=torch.cat([p.flatten(1, 2) for p in poss], 1), mask_flatten=torch.cat([m.flatten(1) for m in masks], 1),
                topk_logits=out["topk_logits"], topk_proposals=out["topk_proposals"])


# ----------------------------------------------------------------------------------------------------------------- the tiny detector
_CACHE = {}


def bert_config():
    cfg = BR.config("a")
    cfg.pop("hidden_dim")
    return cfg


def tiny_state_dict():
    """The tiny detector's state dict under the reference's names, every float a bf16 value (cached; treat as read-only)."""
    if "sd" not in _CACHE:
        g = torch.Generator().manual_seed(31)
        rnd = lambda t: t.to(torch.bfloat16).float()
        unused = tuple(f"norm{i}." for i in range(len(SWIN["depths"])) if i not in SWIN["out_indices"])
        sd = {"backbone.0." + k: v for k, v in SR.seeded_state_dict(SWIN, seed=5).items() if not k.startswith(unused)}
        sd.update(BR.seeded_state_dict(bert_config(), 256, seed=6))
        tw = {k: v for k, v in DR.tower_weights().items() if k != "refpoint_embed.weight"}
        sd.update({"transformer." + k: v for k, v in tw.items()})
        for i in range(DR.GEOM["num_decoder_layers"]):                                             # the shared decoder box head under its top-level alias
            sd.update({f"bbox_embed.{i}." + k[len("decoder.bbox_embed.0."):]: v for k, v in tw.items() if k.startswith("decoder.bbox_embed.0.")})
        chans = [SWIN["embed_dim"] * 2 ** i for i in SWIN["out_indices"]]
        for l, (cin, k) in enumerate([(c, 1) for c in chans] + [(chans[-1], 3)]):
            a = (3.0 / (cin * k * k)) ** 0.5
            sd[f"input_proj.{l}.0.weight"] = rnd((torch.rand(256, cin, k, k, generator=g) * 2 - 1) * a)
            sd[f"input_proj.{l}.0.bias"] = rnd(torch.randn(256, generator=g) * 0.1)
            sd[f"input_proj.{l}.1.weight"] = rnd(0.5 + torch.rand(256, generator=g))
            sd[f"input_proj.{l}.1.bias"] = rnd(torch.randn(256, generator=g) * 0.1)
        _CACHE["sd"] = sd
    return _CACHE["sd"]


def tiny_model(device="cpu", tokenizer=None):
    """anyedit_amd's GroundingDINO at the tiny geometry, filled through the strict loader, in eval mode."""
    from anyedit_amd.checkpoints import load_groundingdino
    from anyedit_amd.groundingdino.backbone import Joiner
    from anyedit_amd.groundingdino.groundingdino import GroundingDINO
    from anyedit_amd.groundingdino.position_encoding import PositionEmbeddingSineHW
    from anyedit_amd.groundingdino.swin_transformer import SwinTransformer
    from anyedit_amd.groundingdino.transformer import Transformer
    g = DR.GEOM
    swin = SwinTransformer(pretrain_img_size=224, **{k: v for k, v in SWIN.items()})
    backbone = Joiner(swin, PositionEmbeddingSineHW(128, temperatureH=TEMPERATURE[0], temperatureW=TEMPERATURE[1], normalize=True))
    backbone.num_channels = [SWIN["embed_dim"] * 2 ** i for i in SWIN["out_indices"]]
    tr = Transformer(d_model=g["d_model"], nhead=g["nhead"], num_queries=g["num_queries"], num_encoder_layers=0, num_decoder_layers=g["num_decoder_layers"],
                     dim_feedforward=g["dff"], dropout=0.0, return_intermediate_dec=True, num_feature_levels=3, learnable_tgt_init=True,
                     two_stage_type="standard", embed_init_tgt=True, use_text_cross_attention=True)
    m = GroundingDINO(backbone, tr, num_queries=g["num_queries"], aux_loss=True, iter_update=True, query_dim=4, num_feature_levels=3, nheads=g["nhead"],
                      two_stage_type="standard", dec_pred_bbox_embed_share=True, two_stage_bbox_embed_share=False, two_stage_class_embed_share=False, dn_number=0,
                      tokenizer=tokenizer or StandInTokenizer(), bert_config=bert_config())
    load_groundingdino(m, dict(tiny_state_dict()))
    return m.eval().requires_grad_(False).to(device)


def tiny_inputs():
    """(pixels fp32 [2, 3, 50, 40] zero-padded, mask bool [2, 50, 40], the two images as a list, tokenized captions)"""
    if "in" not in _CACHE:
        g = torch.Generator().manual_seed(32)
        imgs = [torch.randn(3, h, w, generator=g).to(torch.bfloat16).float() for h, w in SIZES]
        H, W = max(s[0] for s in SIZES), max(s[1] for s in SIZES)
        px, mask = torch.zeros(len(imgs), 3, H, W), torch.ones(len(imgs), H, W, dtype=torch.bool)
        for i, im in enumerate(imgs):
            px[i, :, :im.shape[1], :im.shape[2]] = im
            mask[i, :im.shape[1], :im.shape[2]] = False
        _CACHE["in"] = (px, mask, imgs, StandInTokenizer()(CAPTIONS, padding="longest", return_tensors="pt"))
    return _CACHE["in"]
