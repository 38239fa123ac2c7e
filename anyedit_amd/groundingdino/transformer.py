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
from anyedit_amd.groundingdino.transformer_vanilla import TransformerEncoderLayer, expand_text_mask
from anyedit_amd.groundingdino.utils import _get_activation_fn, _get_clones, get_sine_pos_embed


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
