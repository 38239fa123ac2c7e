"""GroundingDINO/groundingdino/models/GroundingDINO/transformer.py:406-595, :738-799 — the feature enhancer (`Transformer.encoder`) on the HIP path.

Six layers (GroundingDINO_SwinB_cfg.py / GroundingDINO_SwinT_OGC.py), each in the reference's order:

    output, memory_text = fusion_layers[i](output, memory_text, key_padding_mask, text_attention_mask)      fuse_modules.BiAttentionBlock
    memory_text = text_layers[i](memory_text, ~text_self_attention_masks, pos_text)                         transformer_vanilla.TransformerEncoderLayer
    output = layers[i](output, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask)  DeformableTransformerEncoderLayer

Both token streams are bf16 rows between sub-blocks (`# bf16:` marks every stored activation; tests/gdino_enc_ref.py rounds at exactly those points
for its control).  The deformable attention is the existing `MultiScaleDeformableAttention` — its parameters, its fp32 projections (`ops.linear_f32`)
and the `ms_deform_attn` sampling kernel — read in fp32 from the bf16 stream; its fp32 result is added back with one rounding (`ops.scale_residual`).
`forward` returns (output, memory_text) in fp32, as the reference does.

State-dict keys are the reference's (`layers.I.*`, `text_layers.I.*`, `fusion_layers.I.*`), so `checkpoints.load_groundingdino_encoder` fills the
module from the `transformer.encoder.*` entries of a GroundingDINO checkpoint.

Host synchronisation: the level sizes are needed on the host (grid shapes, reference points).  A GPU `spatial_shapes` is read back on every eager
forward, as the reference does; a CPU tensor or a list never synchronises.  A forward runs on the current stream only and may be captured in a
graph: with a CPU `spatial_shapes`, or with the very GPU tensor object of a preceding eager forward (a captured graph replays fixed sizes anyway).
Inference only.
"""
import types
import weakref

import torch
import torch.nn as nn

from anyedit_amd import ops
from anyedit_amd.groundingdino.fuse_modules import BF16, _LN_EPS, BiAttentionBlock, _f32, _mask_u8, as_rows, require_inference
from anyedit_amd.groundingdino.ms_deform_attn import MultiScaleDeformableAttention as MSDeformAttn
from anyedit_amd.groundingdino.transformer_vanilla import TransformerEncoderLayer, _SelfAttnParams, expand_text_mask
from anyedit_amd.groundingdino.utils import MLP, ContrastiveEmbed, _get_activation_fn, _get_clones, get_sine_pos_embed


class DeformableTransformerEncoderLayer(nn.Module):
    """:738-799: src = norm1(src + MSDeformAttn(src + pos, value=src)); src = norm2(src + linear2(relu(linear1(src))))."""

    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % 16 or d_ffn % 8:
            raise ValueError(f"DeformableTransformerEncoderLayer: d_model {d_model} must be a multiple of 16 (ae_linear_f32) and d_ffn {d_ffn} of 8")
        self.self_attn = MSDeformAttn(embed_dim=d_model, num_levels=n_levels, num_heads=n_heads, num_points=n_points, batch_first=True)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation, d_model=d_ffn)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout_rate = dropout
        self.d_model = d_model

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def packed(self):
        ps = (self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias)
        if ops.cache_stale(self, "_pk", *ps):
            self._pk = types.SimpleNamespace(w1=ops.pack_linear(ps[0]), b1=_f32(ps[1]), w2=ops.pack_linear(ps[2]), b2=_f32(ps[3]),
                                             g1=_f32(ps[4]), e1=_f32(ps[5]), g2=_f32(ps[6]), e2=_f32(ps[7]))
        return self._pk

    def _deform(self, x, pos, reference_points, shapes_dev, starts_dev, key_padding_mask, B, N):
        """MultiScaleDeformableAttention.forward (ms_deform_attn.py:231-352, batch_first) on the module's parameters, without its read-back of
        spatial_shapes (the caller has checked that the levels add up to N): fp32 [B*N, C]."""
        a = self.self_attn
        H, L, P = a.num_heads, a.num_levels, a.num_points
        src = x.float()
        q = src if pos is None else src + pos
        lin = lambda m, t: ops.linear_f32(t, m.weight, m.bias)
        v = lin(a.value_proj, src).view(B, N, -1)
        if key_padding_mask is not None:
            v = v.masked_fill(key_padding_mask[..., None], 0.0)
        offsets = lin(a.sampling_offsets, q).view(B, N, H, L, P, 2)
        weights = lin(a.attention_weights, q).view(B, N, H, L * P).softmax(-1).view(B, N, H, L, P)
        loc = a._locations(reference_points, offsets, shapes_dev)
        out = ops.ms_deform_attn(v.view(B, N, H, -1), shapes_dev, starts_dev, loc, weights, a.im2col_step, validated=True)
        return lin(a.output_proj, out.view(B * N, -1))

    def rows_forward(self, x, pos, reference_points, shapes_dev, starts_dev, key_padding_mask, B, N):
        """x: bf16 rows [B*N, C]; pos: fp32 rows [B*N, C] or None.  Returns bf16 rows."""
        pk = self.packed()
        d = self._deform(x, pos, reference_points, shapes_dev, starts_dev, key_padding_mask, B, N)
        y = ops.scale_residual(d, x)                                                  # bf16: :793
        y = ops.layernorm(y, pk.g1, pk.e1, _LN_EPS)                                   # bf16
        h = ops.gemm(y, pk.w1, pk.b1, epilogue=ops.EPI_RELU)                          # bf16
        z = ops.gemm(h, pk.w2, pk.b2, residual=y)                                     # bf16
        return ops.layernorm(z, pk.g2, pk.e2, _LN_EPS)                                # bf16

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask=None):
        require_inference(self, (self.dropout_rate,))
        B, N, C = src.shape
        sizes = _level_sizes(self, spatial_shapes)
        if sum(h * w for h, w in sizes) != N:
            raise ValueError(f"DeformableTransformerEncoderLayer: spatial_shapes {sizes} do not add up to {N} tokens")
        shapes_dev = torch.as_tensor(sizes, dtype=torch.int64).to(src.device) if not (torch.is_tensor(spatial_shapes) and spatial_shapes.is_cuda) else spatial_shapes
        starts_dev = level_start_index.to(src.device)
        p = None if pos is None else pos.detach().float().reshape(B * N, C)
        out = self.rows_forward(as_rows(src), p, reference_points, shapes_dev, starts_dev, key_padding_mask, B, N)
        return out.view(B, N, C).to(src.dtype)


def _level_sizes(mod, spatial_shapes):
    """[(H, W)] on the host.  A CPU tensor or a list never synchronises.  A GPU tensor is read back on EVERY call (the reference reads it too:
    its `get_reference_points` iterates it) — its address and version do not identify its contents, since a caller that builds a fresh tensor
    per image gets the same block back from the caching allocator.  Only while a graph is being captured, where a read-back is impossible, are
    the sizes of the last eager call reused, and only for the very same tensor object (held by weak reference)."""
    if not torch.is_tensor(spatial_shapes):
        return [(int(h), int(w)) for h, w in spatial_shapes]
    if not spatial_shapes.is_cuda:
        return [(int(h), int(w)) for h, w in spatial_shapes.tolist()]
    if torch.cuda.is_current_stream_capturing():
        last = mod.__dict__.get("_sizes_last")
        if last is None or last[0]() is not spatial_shapes or last[2] != ops._version_of(spatial_shapes):
            raise RuntimeError("spatial_shapes is a GPU tensor this module has not seen (unchanged) in its last eager forward: its level sizes cannot be read back during a "
                               "graph capture.  Run one eager forward with the same tensor object first, or pass spatial_shapes as a CPU tensor or a list")
        return last[1]
    sizes = [(int(h), int(w)) for h, w in spatial_shapes.tolist()]
    mod.__dict__["_sizes_last"] = (weakref.ref(spatial_shapes), sizes, ops._version_of(spatial_shapes))
    return sizes


class TransformerEncoder(nn.Module):
    """:406-595 with the reference's constructor and `forward` signature.  `use_checkpoint` / `use_transformer_ckpt` are accepted and change
    nothing at inference.  `tap`, when set to a callable, receives (layer index, sub-block name, output rows, memory_text rows) after every
    sub-block ("fusion", "text", "deform") — what the tests compare against the reference's per-sub-block streams."""

    def __init__(self, encoder_layer, num_layers, d_model=256, num_queries=300, enc_layer_share=False, text_enhance_layer=None, feature_fusion_layer=None,
                 use_checkpoint=False, use_transformer_ckpt=False):
        super().__init__()
        self.layers, self.text_layers, self.fusion_layers = [], [], []
        if num_layers > 0:
            self.layers = _get_clones(encoder_layer, num_layers, layer_share=enc_layer_share)
            if text_enhance_layer is not None:
                self.text_layers = _get_clones(text_enhance_layer, num_layers, layer_share=enc_layer_share)
            if feature_fusion_layer is not None:
                self.fusion_layers = _get_clones(feature_fusion_layer, num_layers, layer_share=enc_layer_share)
        self.query_scale = None
        self.num_queries, self.num_layers, self.d_model = num_queries, num_layers, d_model
        self.use_checkpoint, self.use_transformer_ckpt = use_checkpoint, use_transformer_ckpt
        self.tap = None

    def _dropouts(self):
        """Every dropout / drop-path rate of the sub-blocks (plain floats: one pass, no parameter is touched)."""
        return [r for m in list(self.layers) + list(self.text_layers) + list(self.fusion_layers)
                for r in (getattr(m, "dropout_rate", 0.0), getattr(getattr(m, "attn", None), "dropout", 0.0), getattr(m, "drop_path_rate", 0.0))]

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        """:465-480: the centre of every cell of every level in [0, 1]^2 of the VALID part of the map, then scaled to every level's valid
        ratio: [bs, sum(H W), levels, 2] as (x, y)."""
        pts = []
        for lvl, (H_, W_) in enumerate(spatial_shapes):
            H_, W_ = int(H_), int(W_)
            ys = torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device)
            xs = torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device)
            ref_y, ref_x = torch.meshgrid(ys, xs, indexing="ij")
            ref_y = ref_y.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * H_)
            ref_x = ref_x.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * W_)
            pts.append(torch.stack((ref_x, ref_y), -1))
        reference_points = torch.cat(pts, 1)
        return reference_points[:, :, None] * valid_ratios[:, None]

    def forward(self, src, pos, spatial_shapes, level_start_index, valid_ratios, key_padding_mask, memory_text=None, text_attention_mask=None,
                pos_text=None, text_self_attention_masks=None, position_ids=None):
        """src / pos [bs, sum(H W), C]; spatial_shapes [levels, 2]; level_start_index [levels]; valid_ratios [bs, levels, 2]; key_padding_mask
        bool [bs, sum(H W)], True = padding; memory_text [bs, n_text, C]; text_attention_mask bool [bs, n_text], True = padding;
        text_self_attention_masks bool [bs, n_text, n_text], True = allowed; pos_text [bs, n_text, C] or position_ids [bs, n_text].
        CONTRACT (bi_attention): every sample has an unpadded image token and an unpadded text token; every text row allows a key."""
        require_inference(self, self._dropouts())
        B, Nv, C = src.shape
        dev = src.device
        x = as_rows(src)                                                              # bf16
        posr = None if pos is None else pos.detach().float().reshape(B * Nv, C)
        mask_v = _mask_u8(key_padding_mask, B, Nv, dev)
        kpm = None if key_padding_mask is None else key_padding_mask.to(device=dev, dtype=torch.bool)
        if self.num_layers > 0:
            sizes = _level_sizes(self, spatial_shapes)
            if sum(h * w for h, w in sizes) != Nv:
                raise ValueError(f"TransformerEncoder: spatial_shapes {sizes} do not add up to {Nv} image tokens")
            if torch.is_tensor(spatial_shapes) and spatial_shapes.is_cuda:
                shapes_dev = spatial_shapes
            else:
                key = (tuple(sizes), str(dev))
                if self.__dict__.get("_shapes_key") != key:                           # the device copy is made once per geometry
                    self.__dict__["_shapes_dev"], self.__dict__["_shapes_key"] = torch.as_tensor(sizes, dtype=torch.int64).to(dev), key
                shapes_dev = self.__dict__["_shapes_dev"]
            starts_dev = level_start_index if level_start_index.is_cuda else level_start_index.to(dev)
            reference_points = self.get_reference_points(sizes, valid_ratios.float(), device=dev)
        t = tmask = posb = None
        Nt = 0
        if self.text_layers or self.fusion_layers:
            if memory_text is None:
                raise ValueError("TransformerEncoder: memory_text is required by the text and fusion layers")
            Nt = memory_text.shape[1]
            t = as_rows(memory_text)                                                  # bf16
        if self.text_layers:
            if pos_text is None and position_ids is None:                             # :530-538
                ids = torch.arange(Nt, device=dev).float().unsqueeze(0).unsqueeze(-1).repeat(B, 1, 1)
                pos_text = get_sine_pos_embed(ids, num_pos_feats=256, exchange_xy=False)
            if position_ids is not None:                                              # :539-542: the hard-coded 256 features
                pos_text = get_sine_pos_embed(position_ids[..., None], num_pos_feats=256, exchange_xy=False)
            if pos_text.shape[-1] != C:
                raise ValueError(f"TransformerEncoder: pos_text has {pos_text.shape[-1]} features and d_model is {C} (the reference's position_ids path "
                                 "always makes 256)")
            posb = as_rows(pos_text)                                                  # bf16
            if text_self_attention_masks is None:
                raise ValueError("TransformerEncoder: text_self_attention_masks is required by the text layers (the reference negates it unconditionally)")
            tmask = expand_text_mask(text_self_attention_masks.to(dev), self.text_layers[0].nhead)   # once per forward
        mask_l = _mask_u8(text_attention_mask, B, Nt, dev) if t is not None else None

        for i, layer in enumerate(self.layers):
            if self.fusion_layers:
                x, t = self.fusion_layers[i].rows_forward(x, t, B, Nv, Nt, mask_v, mask_l)
                if self.tap is not None:
                    self.tap(i, "fusion", x, t)
            if self.text_layers:
                t = self.text_layers[i].rows_forward(t, posb, tmask, B, Nt)
                if self.tap is not None:
                    self.tap(i, "text", x, t)
            x = layer.rows_forward(x, posr, reference_points, shapes_dev, starts_dev, kpm, B, Nv)
            if self.tap is not None:
                self.tap(i, "deform", x, t)
        out = x.view(B, Nv, C).float()
        return out, (t.view(B, Nt, C).float() if t is not None else memory_text)


def build_feature_enhancer(d_model=256, nhead=8, dim_feedforward=2048, num_layers=6, num_feature_levels=4, enc_n_points=4, dropout=0.0, text_dropout=0.1,
                           fusion_dropout=0.1, fusion_droppath=0.0):
    """`Transformer.__init__`'s wiring of the encoder (:83-121) with use_text_enhancer = use_fusion_layer = True: the text layer has nhead // 2
    heads and dim_feedforward // 2 hidden units, the fusion has embed_dim = dim_feedforward // 2 over nhead // 2 heads."""
    encoder_layer = DeformableTransformerEncoderLayer(d_model, dim_feedforward, dropout, "relu", num_feature_levels, nhead, enc_n_points)
    text_layer = TransformerEncoderLayer(d_model=d_model, nhead=nhead // 2, dim_feedforward=dim_feedforward // 2, dropout=text_dropout)
    fusion_layer = BiAttentionBlock(v_dim=d_model, l_dim=d_model, embed_dim=dim_feedforward // 2, num_heads=nhead // 2, dropout=fusion_dropout,
                                    drop_path=fusion_droppath)
    return TransformerEncoder(encoder_layer, num_layers, d_model=d_model, text_enhance_layer=text_layer, feature_fusion_layer=fusion_layer)


class DeformableTransformerDecoderLayer(nn.Module):
    """:802-927 in the reference's order: self-attention over the queries (q = k = tgt + query_pos, v = tgt), text cross-attention (optional),
    deformable cross-attention into the image memory, feed-forward; a LayerNorm behind each.  `self_attn` / `ca_text` carry
    nn.MultiheadAttention's parameter names; both run on `ops.attention` at head dim 32."""

    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4, use_text_feat_guide=False,
                 use_text_cross_attention=False):
        super().__init__()
        if use_text_feat_guide:
            raise NotImplementedError("DeformableTransformerDecoderLayer: use_text_feat_guide is not built (the reference asserts it off)")
        if d_model % n_heads or d_model // n_heads != 32:
            raise ValueError(f"DeformableTransformerDecoderLayer: head_dim {d_model}/{n_heads} must be 32 (the attention route the decoder is tested on)")
        if d_model % 16 or d_ffn % 8:
            raise ValueError(f"DeformableTransformerDecoderLayer: d_model {d_model} must be a multiple of 16 and d_ffn {d_ffn} of 8")
        self.cross_attn = MSDeformAttn(embed_dim=d_model, num_levels=n_levels, num_heads=n_heads, num_points=n_points, batch_first=True)
        self.norm1 = nn.LayerNorm(d_model)
        if use_text_cross_attention:
            self.ca_text = _SelfAttnParams(d_model, n_heads)
            self.catext_norm = nn.LayerNorm(d_model)
        self.self_attn = _SelfAttnParams(d_model, n_heads)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation, d_model=d_ffn, batch_dim=1)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.key_aware_proj = None
        self.use_text_feat_guide = use_text_feat_guide
        self.use_text_cross_attention = use_text_cross_attention
        self.dropout_rate, self.d_model, self.n_heads = dropout, d_model, n_heads

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            C = self.d_model
            pk = types.SimpleNamespace()
            a = self.self_attn
            w, b = a.in_proj_weight.detach(), _f32(a.in_proj_bias)
            pk.wqk, pk.bqk, pk.wv, pk.bv = ops.pack_linear(w[:2 * C]), b[:2 * C].contiguous(), ops.pack_linear(w[2 * C:]), b[2 * C:].contiguous()
            pk.wo, pk.bo = ops.pack_linear(a.out_proj.weight), _f32(a.out_proj.bias)
            if self.use_text_cross_attention:
                t = self.ca_text
                w, b = t.in_proj_weight.detach(), _f32(t.in_proj_bias)
                pk.twq, pk.tbq, pk.twkv, pk.tbkv = ops.pack_linear(w[:C]), b[:C].contiguous(), ops.pack_linear(w[C:]), b[C:].contiguous()
                pk.two, pk.tbo = ops.pack_linear(t.out_proj.weight), _f32(t.out_proj.bias)
                pk.gt, pk.et = _f32(self.catext_norm.weight), _f32(self.catext_norm.bias)
            pk.w1, pk.b1, pk.w2, pk.b2 = ops.pack_linear(self.linear1.weight), _f32(self.linear1.bias), ops.pack_linear(self.linear2.weight), _f32(self.linear2.bias)
            pk.g1, pk.e1, pk.g2, pk.e2, pk.g3, pk.e3 = (_f32(t) for t in (self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias,
                                                                           self.norm3.weight, self.norm3.bias))
            self._pk = pk
        return self._pk

    def _deform(self, q, reference_points_input, memory, shapes_dev, starts_dev, key_padding_mask, B, nq, N):
        """MultiScaleDeformableAttention.forward (batch_first) with 4-d reference boxes, on the module's fp32 path: q fp32 rows [B*nq, C] (tgt +
        query_pos), memory fp32 rows [B*N, C] -> fp32 [B*nq, C]."""
        a = self.cross_attn
        H, L, P = a.num_heads, a.num_levels, a.num_points
        lin = lambda m, t: ops.linear_f32(t, m.weight, m.bias)
        v = lin(a.value_proj, memory).view(B, N, -1)
        if key_padding_mask is not None:
            v = v.masked_fill(key_padding_mask[..., None], 0.0)
        offsets = lin(a.sampling_offsets, q).view(B, nq, H, L, P, 2)
        weights = lin(a.attention_weights, q).view(B, nq, H, L * P).softmax(-1).view(B, nq, H, L, P)
        loc = a._locations(reference_points_input, offsets, shapes_dev)
        out = ops.ms_deform_attn(v.view(B, N, H, -1), shapes_dev, starts_dev, loc, weights, a.im2col_step, validated=True)
        return lin(a.output_proj, out.view(B * nq, -1))

    def rows_forward(self, x, qpos, reference_points_input, memory, shapes_dev, starts_dev, key_padding_mask, text, text_live, B, nq, N, Nt):
        """x / qpos: bf16 rows [B*nq, C] (batch-major); memory: fp32 rows [B*N, C]; text: bf16 rows [B*Nt, C]; text_live: uint8 [B, Nt],
        non-zero = a used token (ae_attn_fwd_bf16's sense).  Returns bf16 rows."""
        pk, C, H = self.packed(), self.d_model, self.n_heads
        D = C // H
        qk = ops.gemm(ops.add(x, qpos), pk.wqk, pk.bqk)                               # bf16: q | k of tgt + query_pos (:898)
        v = ops.gemm(x, pk.wv, pk.bv)                                                 # bf16
        a = ops.attention(qk, qk[:, C:], v, B, H, nq, nq, D, D ** -0.5, (nq * 2 * C, D, 2 * C), (nq * 2 * C, D, 2 * C), (nq * C, D, C))   # bf16
        y = ops.gemm(a.view(B * nq, C), pk.wo, pk.bo, residual=x)                     # bf16
        y = ops.layernorm(y, pk.g2, pk.e2, _LN_EPS)                                   # bf16: :901
        if self.use_text_cross_attention:
            q = ops.gemm(ops.add(y, qpos), pk.twq, pk.tbq)                            # bf16
            kv = ops.gemm(text, pk.twkv, pk.tbkv)                                     # bf16: k | v of memory_text
            a = ops.attention(q, kv, kv[:, C:], B, H, nq, Nt, D, D ** -0.5, (nq * C, D, C), (Nt * 2 * C, D, 2 * C), (Nt * 2 * C, D, 2 * C),
                              key_mask=text_live)                                     # bf16
            y = ops.gemm(a.view(B * nq, C), pk.two, pk.tbo, residual=y)               # bf16
            y = ops.layernorm(y, pk.gt, pk.et, _LN_EPS)                               # bf16: :911
        d = self._deform(y.float() + qpos.float(), reference_points_input, memory, shapes_dev, starts_dev, key_padding_mask, B, nq, N)
        y = ops.scale_residual(d, y)                                                  # bf16: :921
        y = ops.layernorm(y, pk.g1, pk.e1, _LN_EPS)                                   # bf16
        h = ops.gemm(y, pk.w1, pk.b1, epilogue=ops.EPI_RELU)                          # bf16
        z = ops.gemm(h, pk.w2, pk.b2, residual=y)                                     # bf16
        return ops.layernorm(z, pk.g3, pk.e3, _LN_EPS)                                # bf16


class TransformerDecoder(nn.Module):
    """:598-735 with the reference's constructor and `forward` signature.  `bbox_embed` / `class_embed` are set by the caller
    (groundingdino.py:163-197).  The isnan / isinf print of :704-713 is a host synchronisation and is left out.  `tap`, when set to a callable,
    receives (layer index, output rows [bs, nq, C] bf16, reference_points fp32 [bs, nq, 4] that entered the layer, query_sine_embed rows)."""

    def __init__(self, decoder_layer, num_layers, norm=None, return_intermediate=False, d_model=256, query_dim=4, num_feature_levels=1):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers) if num_layers > 0 else []
        self.num_layers, self.norm = num_layers, norm
        self.return_intermediate = return_intermediate
        assert return_intermediate, "support return_intermediate only"
        if query_dim != 4:
            raise NotImplementedError("TransformerDecoder: query_dim 2 is not built on the HIP path (GroundingDINO's is 4)")
        if d_model != 256:
            raise ValueError(f"TransformerDecoder: d_model {d_model} must be 256: the sine embedding is 4 x 128 wide into MLP(2 * d_model, ...), so the "
                             "reference itself only runs at 256")
        self.query_dim, self.num_feature_levels, self.d_model = query_dim, num_feature_levels, d_model
        self.ref_point_head = MLP(query_dim // 2 * d_model, d_model, d_model, 2)
        self.query_pos_sine_scale = self.query_scale = self.bbox_embed = self.class_embed = self.ref_anchor_head = None
        self.tap = None

    def _packed(self):
        l0, l1 = self.ref_point_head.layers
        ps = (l0.weight, l0.bias, l1.weight, l1.bias, self.norm.weight, self.norm.bias)
        if ops.cache_stale(self, "_pk", *ps):
            self._pk = types.SimpleNamespace(w0=ops.pack_linear(ps[0]), b0=_f32(ps[1]), w1=ops.pack_linear(ps[2]), b1=_f32(ps[3]), g=_f32(ps[4]), e=_f32(ps[5]))
        return self._pk

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None, pos=None,
                refpoints_unsigmoid=None, level_start_index=None, spatial_shapes=None, valid_ratios=None, memory_text=None, text_attention_mask=None):
        """tgt [nq, bs, C], memory [hw, bs, C], refpoints_unsigmoid [nq, bs, 4], valid_ratios [bs, levels, 2], memory_text [bs, n_text, C],
        text_attention_mask bool [bs, n_text] with True = PADDING (the reference's sense; every sample must keep a token).  `pos` is accepted and
        unused, as in the reference.  Returns [list of [bs, nq, C] fp32, list of [bs, nq, 4] fp32]."""
        if tgt_mask is not None or memory_mask is not None or tgt_key_padding_mask is not None:
            raise NotImplementedError("TransformerDecoder: attention masks over the queries (denoising training) are not built")
        if self.norm is None:
            raise ValueError("TransformerDecoder: norm is required (the reference applies it to every layer's output)")
        require_inference(self, [getattr(m, "dropout_rate", 0.0) for m in self.layers])
        nq, B, C = tgt.shape
        N = memory.shape[0]
        dev = tgt.device
        pk = self._packed()
        sizes = _level_sizes(self, spatial_shapes)
        if sum(h * w for h, w in sizes) != N:
            raise ValueError(f"TransformerDecoder: spatial_shapes {sizes} do not add up to {N} memory tokens")
        if torch.is_tensor(spatial_shapes) and spatial_shapes.is_cuda:
            shapes_dev = spatial_shapes
        else:
            key = (tuple(sizes), str(dev))
            if self.__dict__.get("_shapes_key") != key:
                self.__dict__["_shapes_dev"], self.__dict__["_shapes_key"] = torch.as_tensor(sizes, dtype=torch.int64).to(dev), key
            shapes_dev = self.__dict__["_shapes_dev"]
        starts_dev = level_start_index if level_start_index.is_cuda else level_start_index.to(dev)
        x = as_rows(tgt.transpose(0, 1))                                              # bf16
        mem = memory.detach().transpose(0, 1).float().reshape(B * N, C)
        kpm = None if memory_key_padding_mask is None else memory_key_padding_mask.to(device=dev, dtype=torch.bool)
        text = live = None
        Nt = 0
        if any(l.use_text_cross_attention for l in self.layers):
            Nt = memory_text.shape[1]
            text = as_rows(memory_text)                                               # bf16
            live = (~text_attention_mask.to(device=dev, dtype=torch.bool)).contiguous().view(torch.uint8)   # 0 = masked for ae_attn_fwd_bf16
        vr = valid_ratios.detach().float().contiguous()
        ref = refpoints_unsigmoid.detach().transpose(0, 1).float().sigmoid().contiguous()
        intermediate, ref_points = [], [ref]
        for lid, layer in enumerate(self.layers):
            rpi, sine = ops.gdino_query_sine(ref, vr)                                 # bf16: query_sine_embed (:667-677)
            qpos = ops.gemm(ops.gemm(sine, pk.w0, pk.b0, epilogue=ops.EPI_RELU), pk.w1, pk.b1)   # bf16: ref_point_head, both layers
            x = layer.rows_forward(x, qpos, rpi, mem, shapes_dev, starts_dev, kpm, text, live, B, nq, N, Nt)
            if self.tap is not None:
                self.tap(lid, x.view(B, nq, C), ref, sine)
            if self.bbox_embed is not None:
                ref = self.bbox_embed[lid].refine(x.view(B, nq, C), ref)              # :721-724, on the un-normed stream
                ref_points.append(ref)
            intermediate.append(ops.layernorm(x, pk.g, pk.e, _LN_EPS).view(B, nq, C).float())   # bf16
        return [intermediate, ref_points]


class Transformer(nn.Module):
    """:40-403 with the reference's constructor and `forward(srcs, masks, refpoint_embed, pos_embeds, tgt, attn_mask=None, text_dict=None)`;
    returns (hs, references, hs_enc, ref_enc, init_box_proposal) in fp32 with the reference's shapes.  `enc_out_class_embed`, `enc_out_bbox_embed`,
    `decoder.bbox_embed` and `decoder.class_embed` are attributes the caller sets (groundingdino.py:163-197).  Built: two_stage_type "standard"
    (either embed_init_tgt) and "no" (num_patterns 0), num_encoder_layers 0 (both streams pass through), use_text_cross_attention on or off.
    Ours: the keyword-only `topk_proposals` (int [bs, nq]) replaces the selection (tests, debugging); `last_topk_logits` / `last_topk_proposals` keep the scores
    and the indices of the last forward.  Padded and invalid rows are scored and may be selected, as in the reference; their boxes are sigmoid(+inf) = 1."""

    def __init__(self, d_model=256, nhead=8, num_queries=300, num_encoder_layers=6, num_unicoder_layers=0, num_decoder_layers=6, dim_feedforward=2048,
                 dropout=0.0, activation="relu", normalize_before=False, return_intermediate_dec=False, query_dim=4, num_patterns=0,
                 num_feature_levels=1, enc_n_points=4, dec_n_points=4, learnable_tgt_init=False, two_stage_type="no", embed_init_tgt=False,
                 use_text_enhancer=False, use_fusion_layer=False, use_checkpoint=False, use_transformer_ckpt=False, use_text_cross_attention=False,
                 text_dropout=0.1, fusion_dropout=0.1, fusion_droppath=0.0):
        super().__init__()
        if d_model != 256:
            raise ValueError(f"Transformer: d_model {d_model} must be 256: the sine embedding is 4 x 128 wide into MLP(2 * d_model, ...), so the reference "
                             "itself only runs at 256")
        if not isinstance(num_patterns, int) or num_patterns > 0:
            raise NotImplementedError(f"Transformer: num_patterns={num_patterns} is not built (no GroundingDINO config sets it)")
        if two_stage_type not in ("no", "standard"):
            raise NotImplementedError("unknown param {} of two_stage_type".format(two_stage_type))
        assert query_dim == 4 and not normalize_before
        assert learnable_tgt_init, "why not learnable_tgt_init"
        self.num_feature_levels, self.num_encoder_layers, self.num_unicoder_layers = num_feature_levels, num_encoder_layers, num_unicoder_layers
        self.num_decoder_layers, self.num_queries = num_decoder_layers, num_queries
        encoder_layer = DeformableTransformerEncoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead, enc_n_points)
        text_layer = TransformerEncoderLayer(d_model=d_model, nhead=nhead // 2, dim_feedforward=dim_feedforward // 2, dropout=text_dropout) \
            if use_text_enhancer and num_encoder_layers > 0 else None
        fusion_layer = BiAttentionBlock(v_dim=d_model, l_dim=d_model, embed_dim=dim_feedforward // 2, num_heads=nhead // 2, dropout=fusion_dropout,
                                        drop_path=fusion_droppath) if use_fusion_layer and num_encoder_layers > 0 else None
        self.encoder = TransformerEncoder(encoder_layer, num_encoder_layers, d_model=d_model, num_queries=num_queries, text_enhance_layer=text_layer,
                                          feature_fusion_layer=fusion_layer, use_checkpoint=use_checkpoint, use_transformer_ckpt=use_transformer_ckpt)
        decoder_layer = DeformableTransformerDecoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead, dec_n_points,
                                                          use_text_cross_attention=use_text_cross_attention)
        self.decoder = TransformerDecoder(decoder_layer, num_decoder_layers, nn.LayerNorm(d_model), return_intermediate=return_intermediate_dec,
                                          d_model=d_model, query_dim=query_dim, num_feature_levels=num_feature_levels)
        self.d_model, self.nhead, self.dec_layers, self.num_patterns = d_model, nhead, num_decoder_layers, num_patterns
        self.dropout_rate = dropout
        if num_feature_levels > 1:
            self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model)) if num_encoder_layers > 0 else None
        self.learnable_tgt_init, self.embed_init_tgt = learnable_tgt_init, embed_init_tgt
        if (two_stage_type != "no" and embed_init_tgt) or two_stage_type == "no":
            self.tgt_embed = nn.Embedding(num_queries, d_model)
            nn.init.normal_(self.tgt_embed.weight.data)
        else:
            self.tgt_embed = None
        self.two_stage_type = two_stage_type
        if two_stage_type == "standard":
            self.enc_output = nn.Linear(d_model, d_model)
            self.enc_output_norm = nn.LayerNorm(d_model)
            self.two_stage_wh_embedding = None
        if two_stage_type == "no":
            self.init_ref_points(num_queries)
        self.enc_out_class_embed = None
        self.enc_out_bbox_embed = None
        self.last_topk_logits = self.last_topk_proposals = None
        self._reset_parameters()

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        if self.num_feature_levels > 1 and getattr(self, "level_embed", None) is not None:
            nn.init.normal_(self.level_embed)

    def get_valid_ratio(self, mask):
        _, H, W = mask.shape
        valid_H, valid_W = torch.sum(~mask[:, :, 0], 1), torch.sum(~mask[:, 0, :], 1)
        return torch.stack([valid_W.float() / W, valid_H.float() / H], -1)

    def init_ref_points(self, use_num_queries):
        self.refpoint_embed = nn.Embedding(use_num_queries, 4)

    def _select(self, memory, mask_flatten, sizes, text_dict, topk_proposals):
        """:284-327 on the kernels: proposals; the rows whose keep flag is clear enter enc_output as zeros; enc_output + enc_output_norm; the row
        maximum of the contrastive logits (no logit buffer); stable top-k; gather; enc_out_bbox_embed on the selected rows only (row-wise)."""
        if not isinstance(self.enc_out_class_embed, ContrastiveEmbed) or not isinstance(self.enc_out_bbox_embed, MLP):
            raise RuntimeError("Transformer: two_stage_type='standard' needs enc_out_class_embed (ContrastiveEmbed) and enc_out_bbox_embed (MLP) set by the "
                               "caller, as groundingdino.py:163-197 sets them")
        B, N, C = memory.shape
        ps = (self.enc_output.weight, self.enc_output.bias, self.enc_output_norm.weight, self.enc_output_norm.bias)
        if ops.cache_stale(self, "_pk", *ps):
            self._pk = types.SimpleNamespace(w=ops.pack_linear(ps[0]), b=_f32(ps[1]), g=_f32(ps[2]), e=_f32(ps[3]))
        pk = self._pk
        proposals, keep = ops.gdino_proposals(mask_flatten, sizes)
        rows = as_rows(memory).masked_fill((keep == 0).view(B * N, 1), 0.0)           # bf16: :110-111
        om = ops.layernorm(ops.gemm(rows, pk.w, pk.b), pk.g, pk.e, _LN_EPS)           # bf16: output_memory (:288)
        om = om.view(B, N, C)
        score = self.enc_out_class_embed.rowmax(om, text_dict)                        # :291-295
        self.last_topk_logits = score
        if topk_proposals is None:
            topk_proposals = ops.topk_rows(score, self.num_queries)                   # :301, with a defined order among ties
        idx = topk_proposals.to(device=memory.device, dtype=torch.long)
        self.last_topk_proposals = idx
        if tuple(idx.shape) != (B, self.num_queries):
            raise ValueError(f"Transformer: topk_proposals must be [{B}, {self.num_queries}], got {tuple(idx.shape)}")
        prop_sel = torch.gather(proposals, 1, idx.unsqueeze(-1).expand(-1, -1, 4))
        tgt_undetach = torch.gather(om, 1, idx.unsqueeze(-1).expand(-1, -1, C))
        boxes, unsig = self.enc_out_bbox_embed.refine(tgt_undetach, prop_sel, ref_is_logit=True, want_unsigmoid=True)   # :296-306
        return tgt_undetach.float(), unsig, boxes, prop_sel.sigmoid()

    def forward(self, srcs, masks, refpoint_embed, pos_embeds, tgt, attn_mask=None, text_dict=None, *, topk_proposals=None):
        if refpoint_embed is not None or tgt is not None or attn_mask is not None:
            raise NotImplementedError("Transformer: denoising queries (refpoint_embed / tgt / attn_mask) are a training device and are not built; pass None")
        if text_dict is None:
            raise ValueError("Transformer: text_dict is required (the reference dereferences it unconditionally, :265)")
        require_inference(self, (self.dropout_rate,))
        src_flatten, mask_flatten, pos_flatten, sizes = [], [], [], []
        level_embed = getattr(self, "level_embed", None)
        for lvl, (src, mask, pos_embed) in enumerate(zip(srcs, masks, pos_embeds)):
            bs, c, h, w = src.shape
            sizes.append((h, w))
            p = pos_embed.flatten(2).transpose(1, 2)
            if self.num_feature_levels > 1 and level_embed is not None:
                p = p + level_embed[lvl].view(1, 1, -1)
            src_flatten.append(src.flatten(2).transpose(1, 2))
            mask_flatten.append(mask.flatten(1))
            pos_flatten.append(p)
        src_flatten, mask_flatten, pos_flatten = torch.cat(src_flatten, 1), torch.cat(mask_flatten, 1).contiguous(), torch.cat(pos_flatten, 1)
        valid_ratios = torch.stack([self.get_valid_ratio(m) for m in masks], 1)
        return self.forward_rows(src_flatten, mask_flatten, pos_flatten, sizes, valid_ratios, text_dict, topk_proposals=topk_proposals)

    def forward_rows(self, src_flatten, mask_flatten, pos_flatten, sizes, valid_ratios, text_dict, *, topk_proposals=None):
        """`forward` behind its flattening (:248-403): src_flatten / pos_flatten [bs, sum(h w), C] (pos_flatten already holds `level_embed`),
        mask_flatten bool [bs, sum(h w)] with True = padding, sizes a HOST sequence of (h, w) per level, valid_ratios fp32 [bs, levels, 2].  What
        `ops.gdino_level_geometry` and `ops.gdino_neck_groupnorm` write is taken as it is (bf16 rows are not converted)."""
        if text_dict is None:
            raise ValueError("Transformer: text_dict is required (the reference dereferences it unconditionally, :265)")
        require_inference(self, (self.dropout_rate,))
        sizes = [(int(h), int(w)) for h, w in sizes]
        dev = src_flatten.device
        spatial_shapes = torch.as_tensor(sizes, dtype=torch.long)                     # on the host: never read back
        key = (tuple(sizes), str(dev))
        if self.__dict__.get("_starts_key") != key:                                   # the device copy is made once per geometry (a capture cannot copy from the host)
            starts = torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1]))
            self.__dict__["_starts_dev"], self.__dict__["_starts_key"] = starts.to(dev), key
        level_start_index = self.__dict__["_starts_dev"]
        memory, memory_text = self.encoder(src_flatten, pos=pos_flatten, level_start_index=level_start_index, spatial_shapes=spatial_shapes,
                                           valid_ratios=valid_ratios, key_padding_mask=mask_flatten, memory_text=text_dict["encoded_text"],
                                           text_attention_mask=~text_dict["text_token_mask"], position_ids=text_dict.get("position_ids"),
                                           text_self_attention_masks=text_dict.get("text_self_attention_masks"))
        text_dict["encoded_text"] = memory_text                                       # :279
        bs = memory.shape[0]
        if self.two_stage_type == "standard":
            tgt_undetach, refpoint_embed_, ref_enc, init_box_proposal = self._select(memory, mask_flatten, sizes, text_dict, topk_proposals)
            tgt_ = self.tgt_embed.weight[None].expand(bs, -1, -1) if self.embed_init_tgt else tgt_undetach
            hs_enc, ref_enc = tgt_undetach.unsqueeze(0), ref_enc.unsqueeze(0)
        else:
            tgt_ = self.tgt_embed.weight[None].expand(bs, -1, -1)
            refpoint_embed_ = self.refpoint_embed.weight[None].expand(bs, -1, -1)
            init_box_proposal = refpoint_embed_.detach().float().sigmoid()
            hs_enc = ref_enc = None
        hs, references = self.decoder(tgt=tgt_.transpose(0, 1), memory=memory.transpose(0, 1), memory_key_padding_mask=mask_flatten,
                                      pos=pos_flatten.transpose(0, 1), refpoints_unsigmoid=refpoint_embed_.transpose(0, 1),
                                      level_start_index=level_start_index, spatial_shapes=spatial_shapes, valid_ratios=valid_ratios,
                                      memory_text=text_dict["encoded_text"], text_attention_mask=~text_dict["text_token_mask"])
        return hs, references, hs_enc, ref_enc, init_box_proposal


def build_transformer(args):
    """:930-959."""
    return Transformer(d_model=args.hidden_dim, dropout=args.dropout, nhead=args.nheads, num_queries=args.num_queries, dim_feedforward=args.dim_feedforward,
                       num_encoder_layers=args.enc_layers, num_decoder_layers=args.dec_layers, normalize_before=args.pre_norm, return_intermediate_dec=True,
                       query_dim=args.query_dim, activation=args.transformer_activation, num_patterns=args.num_patterns,
                       num_feature_levels=args.num_feature_levels, enc_n_points=args.enc_n_points, dec_n_points=args.dec_n_points, learnable_tgt_init=True,
                       two_stage_type=args.two_stage_type, embed_init_tgt=args.embed_init_tgt, use_text_enhancer=args.use_text_enhancer,
                       use_fusion_layer=args.use_fusion_layer, use_checkpoint=args.use_checkpoint, use_transformer_ckpt=args.use_transformer_ckpt,
                       use_text_cross_attention=args.use_text_cross_attention, text_dropout=args.text_dropout, fusion_dropout=args.fusion_dropout,
                       fusion_droppath=args.fusion_droppath)


def prediction_heads(hs, references, bbox_embed, class_embed, text_dict, aux=False):
    """groundingdino.py:317-335, the box and contrastive heads behind the decoder: hs a sequence of [bs, nq, 256] (the decoder's NORMED outputs, one
    per layer), references a sequence of one more sigmoid box tensor [bs, nq, 4] (the last is unused, as `reference[:-1]` there), bbox_embed /
    class_embed sequences of `utils.MLP` / `utils.ContrastiveEmbed` per layer.  Returns {"pred_logits": fp32 [bs, nq, max_text_len], "pred_boxes":
    fp32 [bs, nq, 4]} of the last layer; with aux=True also "aux_outputs", the same pair for every earlier layer (`_set_aux_loss`).  Note that the
    decoder's own refinement applies bbox_embed to the un-normed stream: that is another call."""
    n = len(hs)
    if n < 1 or len(references) != n + 1 or len(bbox_embed) < n or len(class_embed) < n:
        raise ValueError(f"prediction_heads: {n} decoder outputs need {n + 1} references and {n} box / class heads, got {len(references)}, "
                         f"{len(bbox_embed)}, {len(class_embed)}")
    one = lambda l: {"pred_logits": class_embed[l](hs[l], text_dict), "pred_boxes": bbox_embed[l].refine(hs[l], references[l])}
    out = one(n - 1)
    if aux:
        out["aux_outputs"] = [one(l) for l in range(n - 1)]
    return out
