"""GroundingDINO/groundingdino/models/GroundingDINO/groundingdino.py:51-349, :363-395 — the detector on the HIP path.

`GroundingDINO` (below `GroundingDINOText`, whose text logic and `bert.*` / `feat_map.*` keys it inherits) joins the towers:

    ws = backbone[0].run(pixels)                                                                   swin_transformer.SwinTransformer
    per backbone level:  u = ops.gemm(stage.z, W_l, b_l, out_f32=True)                             input_proj[l][0], a 1x1 conv on the normed rows  (:295)
                         ops.gdino_neck_groupnorm(u, ..., out=src_flatten, row_offset=start_l)     input_proj[l][1], into the concatenated buffer
    per extra level:     u = ops.conv3x3(rows, W_l, b_l, stride=2, out_f32=True); the same norm     (:298-310)
    mask_flatten, pos_flatten, valid_ratios = ops.gdino_level_geometry(mask, sizes, level_embed)   (:306-307, backbone.py:113, position_encoding.py)
    hs, references, ... = transformer.forward_rows(src_flatten, mask_flatten, pos_flatten, ...)    (:313)
    prediction_heads(hs, references, bbox_embed, class_embed, text_dict)                           (:317-335)

No NCHW map is made between the tower and the transformer.  After the first call of a shape `detect` keeps no buffer of its own that it did
not have before and never synchronises with the host; it runs on the current stream and may be captured in a graph.

The text side (:106-119 and :233-283): a caption goes in, the `text_dict` that `transformer.Transformer` reads comes out.

    tokenized = tokenizer(captions, padding="longest")                                            host (the caller's tokenizer)
    spans, position_ids, text_self_attention_masks = sub-sentence rule(input_ids)                 ops.gdino_text_spans       (:237-243)
    truncation to max_text_len                                                                    copies into static buffers (:245-252)
    last_hidden_state = bert(input_ids, token_type_ids, position_ids, key_spans=spans)            bertwarper.BertModel       (:255-263)
    encoded_text = feat_map(last_hidden_state)                                                    ops.gemm                   (:265)      # bf16

`GroundingDINOText` holds `bert` and `feat_map` under the checkpoint's names.  The tokenizer is an object the caller passes in: nothing here reaches for a network.

`encoded_text` is bf16, the dtype `Transformer.forward` turns its text rows into (`as_rows`), so no conversion launch sits between the two.
After the first call at a given (B, N) `encode_tokenized` makes no allocation and no host synchronisation when its inputs are already on the
GPU, runs on the current stream only (no parallel branches) and may be captured in a graph; the four returned tensors are static per shape.
"""
import copy
import types

import torch
import torch.nn as nn

from anyedit_amd import ops
from anyedit_amd.groundingdino.bertwarper import MAX_TOKENS, BertModel, BertModelWarper
from anyedit_amd.groundingdino.fuse_modules import require_inference
from anyedit_amd.groundingdino.misc import NestedTensor
from anyedit_amd.groundingdino.utils import MLP, ContrastiveEmbed

BF16 = torch.bfloat16
SPECIAL_TOKENS = ["[CLS]", "[SEP]", ".", "?"]           # groundingdino.py:119


class GroundingDINOText(nn.Module):
    def __init__(self, bert_config=None, hidden_dim=256, tokenizer=None, max_text_len=256, sub_sentence_present=True, special_token_ids=None):
        """bert_config: dict over `bertwarper.BERT_BASE`; tokenizer: any object with the Hugging Face call signature and `convert_tokens_to_ids`
        (or pass `special_token_ids`, the ids of "[CLS]", "[SEP]", ".", "?", and call `encode_tokenized` yourself)."""
        super().__init__()
        if not 1 <= max_text_len <= MAX_TOKENS:
            raise ValueError(f"GroundingDINOText: max_text_len {max_text_len} outside [1, {MAX_TOKENS}]")
        if hidden_dim % 8:
            raise ValueError(f"GroundingDINOText: hidden_dim {hidden_dim} must be a multiple of 8")
        self.bert = BertModelWarper(BertModel(bert_config))
        self.feat_map = nn.Linear(self.bert.config["hidden_size"], hidden_dim, bias=True)
        nn.init.constant_(self.feat_map.bias.data, 0)
        nn.init.xavier_uniform_(self.feat_map.weight.data)
        self.hidden_dim = hidden_dim
        self.tokenizer = tokenizer
        self.max_text_len = max_text_len
        self.sub_sentence_present = sub_sentence_present
        if special_token_ids is None:
            if tokenizer is None:
                raise ValueError("GroundingDINOText: pass tokenizer= (an object with convert_tokens_to_ids) or special_token_ids=; nothing is ever downloaded")
            special_token_ids = tokenizer.convert_tokens_to_ids(SPECIAL_TOKENS)
        self.specical_tokens = [int(t) for t in special_token_ids]           # the reference's spelling
        if len(self.specical_tokens) > 8:
            raise ValueError("GroundingDINOText: at most 8 special token ids")
        self._ws = {}

    def _packed(self):
        f = self.feat_map
        if ops.cache_stale(self, "_pk", f.weight, f.bias):
            self._pk = types.SimpleNamespace(w=ops.pack_linear(f.weight), b=f.bias.detach().float().contiguous())
        return self._pk

    def _workspace(self, B, N0, N, dev):
        key = (B, N0, N, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev)
            ws = self._ws[key] = types.SimpleNamespace(
                ids=z(B, N0, dt=torch.int64), tids=z(B, N0, dt=torch.int64), amask=z(B, N0, dt=torch.bool), spans=z(B, N0, 2, dt=torch.int32),
                pos=z(B, N0, dt=torch.int64), mask=z(B, N0, N0, dt=torch.bool), enc=z(B, N, self.hidden_dim, dt=BF16))
            if N != N0:
                ws.ids_t, ws.tids_t, ws.amask_t = z(B, N, dt=torch.int64), z(B, N, dt=torch.int64), z(B, N, dt=torch.bool)
                ws.spans_t, ws.pos_t, ws.mask_t = z(B, N, 2, dt=torch.int32), z(B, N, dt=torch.int64), z(B, N, N, dt=torch.bool)
        return ws

    @staticmethod
    def _in(t, buf):
        """A GPU tensor of the buffer's dtype is used in place; anything else (a tokenizer's CPU tensors) is copied into the static buffer."""
        t = torch.as_tensor(t)
        if t.is_cuda and t.dtype == buf.dtype and t.is_contiguous() and t.device == buf.device:
            return t
        buf.copy_(t)
        return buf

    @torch.no_grad()
    def encode_tokenized(self, tokenized):
        """groundingdino.py:237-283.  tokenized: a mapping with `input_ids` [B, N0] and `attention_mask` [B, N0] (`token_type_ids` optional: zeros),
        on the host or the GPU, N0 <= 256, column 0 of every row a special token ([CLS]).  Returns the text_dict: `encoded_text` bf16
        [B, N, hidden_dim], `text_token_mask` bool [B, N], `position_ids` long [B, N], `text_self_attention_masks` bool [B, N, N], with
        N = min(N0, max_text_len); static per shape (overwritten by the next call of that shape)."""
        dev = self.feat_map.weight.device
        if dev.type != "cuda":
            raise ValueError("GroundingDINOText: the encoder runs on the GPU only (anyedit_amd has no CPU path); move it with .to('cuda')")
        ids = torch.as_tensor(tokenized["input_ids"])
        if ids.dim() != 2 or ids.numel() == 0:
            raise ValueError(f"GroundingDINOText: input_ids of shape {tuple(ids.shape)}; expected [B, N]")
        if not ids.is_cuda:
            self.bert.__dict__["_model"]._check_host_ids(ids)
        B, N0 = ids.shape
        if N0 > MAX_TOKENS:
            raise ValueError(f"GroundingDINOText: {N0} tokens; the sub-sentence rule runs on at most {MAX_TOKENS} (truncate the caption in the tokenizer)")
        N = min(N0, self.max_text_len)
        ws = self._workspace(B, N0, N, dev)
        ids = self._in(ids, ws.ids)
        amask = self._in(tokenized["attention_mask"], ws.amask)
        tt = tokenized.get("token_type_ids") if hasattr(tokenized, "get") else tokenized["token_type_ids"]
        tids = None if tt is None else self._in(tt, ws.tids)
        spans, pos, mask = ops.gdino_text_spans(ids, self.specical_tokens, spans=ws.spans, position_ids=ws.pos, dense_mask=ws.mask)   # :237-243
        if N != N0:                                                                    # :245-252
            ws.ids_t.copy_(ids[:, :N])
            ws.amask_t.copy_(amask[:, :N])
            ws.pos_t.copy_(pos[:, :N])
            ws.mask_t.copy_(mask[:, :N, :N])
            torch.clamp(spans[:, :N], max=N, out=ws.spans_t)                           # a span cut by the truncation keeps its keys below N
            ids, amask, pos, mask, spans = ws.ids_t, ws.amask_t, ws.pos_t, ws.mask_t, ws.spans_t
            if tids is not None:
                ws.tids_t.copy_(tids[:, :N])
                tids = ws.tids_t
        if self.sub_sentence_present:                                                  # :255-263
            out = self.bert(input_ids=ids, token_type_ids=tids, position_ids=pos, key_spans=spans, output_pooler=False)
        else:
            out = self.bert(input_ids=ids, token_type_ids=tids, attention_mask=amask, output_pooler=False)
        pk = self._packed()
        C = self.bert.config["hidden_size"]
        ops.gemm(out.last_hidden_state.view(B * N, C), pk.w, pk.b, out=ws.enc.view(B * N, self.hidden_dim))      # bf16: feat_map (:265)
        return {"encoded_text": ws.enc, "text_token_mask": amask, "position_ids": pos, "text_self_attention_masks": mask}

    def forward(self, captions):
        """captions: list of strings -> the text_dict (fresh tensors)."""
        if self.tokenizer is None:
            raise ValueError("GroundingDINOText has no tokenizer: pass tokenizer=<object with the Hugging Face call signature>, or tokenize "
                             "yourself and call encode_tokenized(tokenized); nothing is ever downloaded")
        tokenized = self.tokenizer(captions, padding="longest", return_tensors="pt")   # :234
        return {k: v.clone() for k, v in self.encode_tokenized(tokenized).items()}


def nested_tensor_from_tensor_list(tensor_list):
    """util/misc.py:283-320: [3, h_i, w_i] images -> one zero-padded batch and its mask (True on padding).  A [B, 3, H, W] tensor has no padding
    (mask None)."""
    if isinstance(tensor_list, torch.Tensor):
        if tensor_list.dim() != 4:
            raise ValueError(f"GroundingDINO: a tensor of images must be [B, 3, H, W], got {tuple(tensor_list.shape)}")
        return NestedTensor(tensor_list.contiguous(), None)
    if not tensor_list or any(t.dim() != 3 for t in tensor_list):
        raise ValueError("GroundingDINO: a list of images must hold [3, h, w] tensors")
    H, W = max(t.shape[1] for t in tensor_list), max(t.shape[2] for t in tensor_list)
    t0 = tensor_list[0]
    batch = torch.zeros(len(tensor_list), t0.shape[0], H, W, dtype=t0.dtype, device=t0.device)
    mask = torch.ones(len(tensor_list), H, W, dtype=torch.bool, device=t0.device)
    for img, pad, m in zip(tensor_list, batch, mask):
        pad[:, :img.shape[1], :img.shape[2]].copy_(img)
        m[:img.shape[1], :img.shape[2]] = False
    return NestedTensor(batch, mask)


class GroundingDINO(GroundingDINOText):
    """:51-349 with the reference's constructor arguments and its wiring of the box and class heads.  Ours, keyword only: `tokenizer` (the object
    the reference would download; `text_encoder_type` is kept as a name and never resolved), `bert_config` (a dict over `bertwarper.BERT_BASE`)
    and `special_token_ids`.  Not built: num_feature_levels == 1, training targets, denoising queries."""

    def __init__(self, backbone, transformer, num_queries, aux_loss=False, iter_update=False, query_dim=2, num_feature_levels=1, nheads=8,
                 two_stage_type="no", dec_pred_bbox_embed_share=True, two_stage_class_embed_share=True, two_stage_bbox_embed_share=True, num_patterns=0,
                 dn_number=100, dn_box_noise_scale=0.4, dn_label_noise_ratio=0.5, dn_labelbook_size=100, text_encoder_type="bert-base-uncased",
                 sub_sentence_present=True, max_text_len=256, *, tokenizer=None, bert_config=None, special_token_ids=None):
        hidden_dim = transformer.d_model
        super().__init__(bert_config=bert_config, hidden_dim=hidden_dim, tokenizer=tokenizer, max_text_len=max_text_len,
                         sub_sentence_present=sub_sentence_present, special_token_ids=special_token_ids)
        assert query_dim == 4
        assert iter_update, "Why not iter_update?"
        if num_feature_levels <= 1:
            raise NotImplementedError("GroundingDINO: num_feature_levels == 1 is not built (every public config has 4 levels; the single-level form has no "
                                      "level embedding and two_stage_type 'no')")
        if dn_number:
            raise NotImplementedError("GroundingDINO: denoising queries (dn_number > 0) are a training device and are not built; build_groundingdino passes 0")
        if hidden_dim != ops.NECK_GN_C:
            raise ValueError(f"GroundingDINO: hidden_dim {hidden_dim} must be {ops.NECK_GN_C} (ae_gdino_neck_groupnorm, the sine embedding)")
        if max_text_len % 32 or max_text_len > ops.GROUND_MAX_TEXT:
            raise ValueError(f"GroundingDINO: max_text_len {max_text_len} must be a multiple of 32 up to {ops.GROUND_MAX_TEXT} (ae_gdino_ground's token bit sets)")
        num_backbone_outs = len(backbone.num_channels)
        if num_feature_levels < num_backbone_outs or num_feature_levels != transformer.num_feature_levels:
            raise ValueError(f"GroundingDINO: {num_feature_levels} levels against {num_backbone_outs} backbone outputs and the transformer's "
                             f"{transformer.num_feature_levels}")
        self.num_queries, self.transformer, self.hidden_dim, self.num_feature_levels, self.nheads = num_queries, transformer, hidden_dim, num_feature_levels, nheads
        self.query_dim, self.num_patterns, self.text_encoder_type = query_dim, num_patterns, text_encoder_type
        self.dn_number, self.dn_box_noise_scale, self.dn_label_noise_ratio, self.dn_labelbook_size = dn_number, dn_box_noise_scale, dn_label_noise_ratio, dn_labelbook_size
        proj = []                                                                      # :122-141
        in_channels = None
        for c in backbone.num_channels:
            in_channels = c
            proj.append(nn.Sequential(nn.Conv2d(in_channels, hidden_dim, kernel_size=1), nn.GroupNorm(32, hidden_dim)))
        for _ in range(num_feature_levels - num_backbone_outs):
            proj.append(nn.Sequential(nn.Conv2d(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1), nn.GroupNorm(32, hidden_dim)))
            in_channels = hidden_dim
        self.input_proj = nn.ModuleList(proj)
        self.backbone = backbone
        self.aux_loss, self.box_pred_damping, self.iter_update = aux_loss, None, iter_update
        self.dec_pred_bbox_embed_share = dec_pred_bbox_embed_share
        _class_embed = ContrastiveEmbed(max_text_len)                                  # :163-197
        _bbox_embed = MLP(hidden_dim, hidden_dim, 4, 3)
        nn.init.constant_(_bbox_embed.layers[-1].weight.data, 0)
        nn.init.constant_(_bbox_embed.layers[-1].bias.data, 0)
        n_dec = transformer.num_decoder_layers
        self.bbox_embed = nn.ModuleList([_bbox_embed if dec_pred_bbox_embed_share else copy.deepcopy(_bbox_embed) for _ in range(n_dec)])
        self.class_embed = nn.ModuleList([_class_embed for _ in range(n_dec)])
        self.transformer.decoder.bbox_embed = self.bbox_embed
        self.transformer.decoder.class_embed = self.class_embed
        self.two_stage_type = two_stage_type
        assert two_stage_type in ["no", "standard"], "unknown param {} of two_stage_type".format(two_stage_type)
        if two_stage_type != "no":
            if two_stage_bbox_embed_share:
                assert dec_pred_bbox_embed_share
                self.transformer.enc_out_bbox_embed = _bbox_embed
            else:
                self.transformer.enc_out_bbox_embed = copy.deepcopy(_bbox_embed)
            if two_stage_class_embed_share:
                assert dec_pred_bbox_embed_share
                self.transformer.enc_out_class_embed = _class_embed
            else:
                self.transformer.enc_out_class_embed = copy.deepcopy(_class_embed)
            self.refpoint_embed = None
        self._neck = {}
        self.last_src_flatten = self.last_pos_flatten = self.last_mask_flatten = None
        for p in self.input_proj:                                                      # :203-207
            nn.init.xavier_uniform_(p[0].weight, gain=1)
            nn.init.constant_(p[0].bias, 0)

    # ---- the neck -------------------------------------------------------------------------------------------------------------
    def _proj_packed(self):
        ps = [t for p in self.input_proj for t in (p[0].weight, p[0].bias, p[1].weight, p[1].bias)]
        le = getattr(self.transformer, "level_embed", None)
        if ops.cache_stale(self, "_ppk", *ps, le):
            f32 = lambda t: t.detach().float().contiguous()
            pk = []
            for p in self.input_proj:
                conv, gn = p[0], p[1]
                if conv.kernel_size == (1, 1):
                    w = ops.pack_linear(conv.weight.view(conv.out_channels, conv.in_channels))
                else:
                    w = ops.pack_conv3x3(conv.weight.detach())
                pk.append(types.SimpleNamespace(w=w, b=f32(conv.bias), g=f32(gn.weight), e=f32(gn.bias), eps=gn.eps))
            self._ppk = types.SimpleNamespace(levels=pk, level_embed=None if le is None else f32(le))
        return self._ppk

    def level_sizes(self, H, W):
        """[(h, w)] of every feature level for an H x W batch: the tower's out_indices stages, then the stride-2 levels."""
        tower = self.backbone[0]
        stages = tower.stage_sizes(H, W)
        sizes = [stages[i] for i in range(tower.num_layers) if i in tower.out_indices]
        for _ in range(self.num_feature_levels - len(sizes)):
            h, w = sizes[-1]
            sizes.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
        return sizes

    def _neck_workspace(self, B, H, W, dev):
        key = (B, H, W, str(dev))
        ws = self._neck.get(key)
        if ws is None:
            sizes = self.level_sizes(H, W)
            N, L, C = sum(h * w for h, w in sizes), len(sizes), self.hidden_dim
            starts = [sum(h * w for h, w in sizes[:l]) for l in range(L)]
            e = lambda *s, dt: torch.empty(*s, dtype=dt, device=dev)
            ws = self._neck[key] = types.SimpleNamespace(
                sizes=sizes, starts=starts, N=N, src=e(B, N, C, dt=BF16), pos=e(B, N, C, dt=BF16), mask=e(B, N, dt=torch.bool), vr=e(B, L, 2, dt=torch.float32),
                u=[e(B * h * w, C, dt=torch.float32) for h, w in sizes], gn=[ops.gdino_neck_groupnorm_workspace(B, h * w, dev) for h, w in sizes],
                rows=[e(B * h * w, C, dt=BF16) for h, w in sizes])
        return ws

    def neck(self, stages, mask, B, H, W):
        """input_proj and the level geometry: the tower's workspace stages -> the neck workspace (src / pos / mask / vr / sizes)."""
        tower, pe = self.backbone[0], self.backbone[1]
        pe.check_built()
        pk = self._proj_packed()
        dev = stages[0].x0.device
        ws = self._neck_workspace(B, H, W, dev)
        outs = [i for i in range(tower.num_layers) if i in tower.out_indices]
        for l, pl in enumerate(pk.levels):
            h, w = ws.sizes[l]
            if l < len(outs):
                ops.gemm(stages[outs[l]].z, pl.w, pl.b, out_f32=True, out=ws.u[l])                                   # fp32: :295, the 1x1 conv
            else:
                ph, pw = ws.sizes[l - 1]
                if l == len(outs):
                    rows = stages[outs[-1]].z                                                                        # :302: the last backbone map
                else:
                    rows = ws.rows[l - 1]                                                                            # :304: the previous level's output
                    rows.view(B, ph * pw, -1).copy_(ws.src[:, ws.starts[l - 1]:ws.starts[l - 1] + ph * pw])
                _, ho, wo = ops.conv3x3(rows, pl.w, pl.b, B, ph, pw, stride=2, out_f32=True, out=ws.u[l])            # fp32
                assert (ho, wo) == (h, w)
            ops.gdino_neck_groupnorm(ws.u[l], pl.g, pl.e, B, h * w, pl.eps, out=ws.src, row_offset=ws.starts[l], workspace=ws.gn[l])   # bf16: src_flatten
        ops.gdino_level_geometry(mask, ws.sizes, B, pe.temperatureH, pe.temperatureW, pk.level_embed, device=dev, mask_flatten=ws.mask, pos_flatten=ws.pos,
                                 valid_ratios=ws.vr)                                                                 # bf16: pos_flatten
        return ws

    # ---- the detector ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def detect(self, pixels, mask, tokenized, *, topk_proposals=None):
        """The device part of `forward`: pixels [B, 3, H, W] fp32 / bf16 and mask bool [B, H, W] (or None: nothing padded) on the GPU, `tokenized`
        as `encode_tokenized` takes it.  With the token tensors already on the GPU nothing here synchronises with the host.  The returned
        tensors are fresh; `last_src_flatten` / `last_pos_flatten` / `last_mask_flatten` are the static neck buffers of this shape."""
        require_inference(self)
        B, _, H, W = pixels.shape
        if mask is not None and tuple(mask.shape) != (B, H, W):
            raise ValueError(f"GroundingDINO: mask of shape {tuple(mask.shape)} for pixels {tuple(pixels.shape)}")
        text_dict = dict(self.encode_tokenized(tokenized))
        tws = self.backbone[0].run(pixels)
        ws = self.neck(tws.stages, mask, B, H, W)
        self.last_src_flatten, self.last_pos_flatten, self.last_mask_flatten = ws.src, ws.pos, ws.mask
        hs, references, _, _, _ = self.transformer.forward_rows(ws.src, ws.mask, ws.pos, ws.sizes, ws.vr, text_dict, topk_proposals=topk_proposals)
        from anyedit_amd.groundingdino.transformer import prediction_heads
        return prediction_heads(hs, references, self.bbox_embed, self.class_embed, text_dict)

    def forward(self, samples, targets=None, *, topk_proposals=None, **kw):
        """:212-349.  samples: a NestedTensor, a [B, 3, H, W] tensor or a list of [3, h, w] tensors (padded to a common size with a mask);
        captions=[...] one per image.  Returns {"pred_logits": fp32 [B, num_queries, max_text_len], "pred_boxes": fp32 [B, num_queries, 4]}."""
        if targets is not None:
            raise NotImplementedError("GroundingDINO: training targets are not built (inference only); pass captions=[...]")
        if "captions" not in kw:
            raise ValueError("GroundingDINO.forward: pass captions=[...], one per image")
        captions = list(kw["captions"])
        if self.tokenizer is None:
            raise ValueError("GroundingDINO has no tokenizer: pass tokenizer=<object with the Hugging Face call signature> to the constructor, or tokenize "
                             "yourself and call detect(pixels, mask, tokenized); nothing is ever downloaded")
        if isinstance(samples, (list, tuple, torch.Tensor)):
            samples = nested_tensor_from_tensor_list(samples)
        dev = self.feat_map.weight.device
        pixels = samples.tensors.to(dev).contiguous()
        mask = None if samples.mask is None else samples.mask.to(dev)
        if len(captions) != pixels.shape[0]:
            raise ValueError(f"GroundingDINO.forward: {len(captions)} captions for {pixels.shape[0]} images")
        tokenized = self.tokenizer(captions, padding="longest", return_tensors="pt")   # :234
        return self.detect(pixels, mask, tokenized, topk_proposals=topk_proposals)


def build_groundingdino(args, tokenizer=None):
    """:363-395.  `tokenizer`: the object the reference would fetch by `args.text_encoder_type`; `args.bert_config` (optional) overrides BERT-base."""
    from anyedit_amd.groundingdino.backbone import build_backbone
    from anyedit_amd.groundingdino.transformer import build_transformer
    backbone = build_backbone(args)
    transformer = build_transformer(args)
    return GroundingDINO(backbone, transformer, num_queries=args.num_queries, aux_loss=True, iter_update=True, query_dim=4,
                         num_feature_levels=args.num_feature_levels, nheads=args.nheads, dec_pred_bbox_embed_share=args.dec_pred_bbox_embed_share,
                         two_stage_type=args.two_stage_type, two_stage_bbox_embed_share=args.two_stage_bbox_embed_share,
                         two_stage_class_embed_share=args.two_stage_class_embed_share, num_patterns=args.num_patterns, dn_number=0,
                         dn_box_noise_scale=args.dn_box_noise_scale, dn_label_noise_ratio=args.dn_label_noise_ratio, dn_labelbook_size=args.dn_labelbook_size,
                         text_encoder_type=args.text_encoder_type, sub_sentence_present=args.sub_sentence_present, max_text_len=args.max_text_len,
                         tokenizer=tokenizer, bert_config=getattr(args, "bert_config", None))
