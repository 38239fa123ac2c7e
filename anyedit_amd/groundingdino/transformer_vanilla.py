"""GroundingDINO/groundingdino/models/GroundingDINO/transformer_vanilla.py:72-123 — the text self-attention layer of the feature enhancer on HIP.

Post-norm, ReLU, q = k = src + pos, v = src; bf16 rows [B*N, C] (batch-major) between launches:

    qk_in = x + pos                                        ops.add                       # bf16
    q | k = qk_in in_proj[:2C]^T,  v = x in_proj[2C:]^T    ops.gemm (+bias)              # bf16
    a = softmax(scale q k^T, disallowed keys removed) v    ops.attention_masked_short    # bf16
    y = norm1(x + a out_proj^T + b)                        ops.gemm (residual), ops.layernorm
    out = norm2(y + relu(y W1^T + b1) W2^T + b2)           ops.gemm (EPI_RELU), ops.gemm (residual), ops.layernorm

The parameters carry nn.MultiheadAttention's names (`self_attn.in_proj_weight`, `self_attn.in_proj_bias`, `self_attn.out_proj.weight / bias`), so
the `text_layers.*` entries of a GroundingDINO checkpoint load unchanged.

The reference's mask indexing is reproduced: it calls `src_mask.repeat(self.nhead, 1, 1)` (:111), which tiles the BATCH axis, while
nn.MultiheadAttention reads slice b * nhead + h for (sample b, head h) — so that pair attends under the mask of sample (b * nhead + h) mod bs.
`expand_text_mask` builds the [bs * nhead, N, N] uint8 "allowed" mask in that order.
"""
import types

import torch
import torch.nn as nn

from anyedit_amd import ops
from anyedit_amd.groundingdino.fuse_modules import BF16, _LN_EPS, _f32, as_rows, require_inference
from anyedit_amd.groundingdino.utils import _get_activation_fn


def expand_text_mask(allowed, nhead):
    """allowed: bool [bs, N, N], True = query row i may attend key j (text_self_attention_masks, before the `~` of transformer.py:569) ->
    uint8 [bs * nhead, N, N] where slice b * nhead + h is allowed[(b * nhead + h) % bs]: the reference's `repeat(nhead, 1, 1)`."""
    bs = allowed.shape[0]
    idx = torch.arange(bs * nhead, device=allowed.device) % bs
    return allowed.to(torch.bool)[idx].contiguous().view(torch.uint8)


class _SelfAttnParams(nn.Module):
    """The parameters of nn.MultiheadAttention(d_model, nhead) under its names; the attention itself runs in the layer."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.0)


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", normalize_before=False):
        super().__init__()
        if normalize_before:
            raise NotImplementedError("TransformerEncoderLayer: normalize_before=True is not built (the reference's forward never reads it)")
        if d_model % nhead or d_model // nhead not in (32, 64):
            raise ValueError(f"TransformerEncoderLayer: head_dim {d_model}/{nhead} must be 32 or 64 (ae_attn_masked_short_bf16)")
        if d_model % 8 or dim_feedforward % 8:
            raise ValueError(f"TransformerEncoderLayer: d_model {d_model} and dim_feedforward {dim_feedforward} must be multiples of 8")
        self.self_attn = _SelfAttnParams(d_model, nhead)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.activation = _get_activation_fn(activation)
        self.dropout_rate = dropout
        self.normalize_before = normalize_before
        self.nhead = nhead
        self.d_model = d_model

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            a, C = self.self_attn, self.d_model
            w, b = a.in_proj_weight.detach(), _f32(a.in_proj_bias)
            self._pk = types.SimpleNamespace(wqk=ops.pack_linear(w[:2 * C]), bqk=b[:2 * C].contiguous(), wv=ops.pack_linear(w[2 * C:]), bv=b[2 * C:].contiguous(),
                                             wo=ops.pack_linear(a.out_proj.weight), bo=_f32(a.out_proj.bias),
                                             w1=ops.pack_linear(self.linear1.weight), b1=_f32(self.linear1.bias),
                                             w2=ops.pack_linear(self.linear2.weight), b2=_f32(self.linear2.bias),
                                             g1=_f32(self.norm1.weight), e1=_f32(self.norm1.bias), g2=_f32(self.norm2.weight), e2=_f32(self.norm2.bias))
        return self._pk

    def rows_forward(self, x, pos, mask, B, N):
        """x: bf16 rows [B*N, C] (batch-major); pos: bf16 rows or None; mask: `expand_text_mask` output.  Returns bf16 rows."""
        pk, C, H = self.packed(), self.d_model, self.nhead
        D = C // H
        qk_in = x if pos is None else ops.add(x, pos)                                 # bf16
        qk = ops.gemm(qk_in, pk.wqk, pk.bqk)                                          # bf16: q | k
        v = ops.gemm(x, pk.wv, pk.bv)                                                 # bf16
        a = ops.attention_masked_short(qk, qk[:, C:], v, mask, B, H, N, D, D ** -0.5, (N * 2 * C, D, 2 * C), (N * 2 * C, D, 2 * C), (N * C, D, C))   # bf16
        y = ops.gemm(a.view(B * N, C), pk.wo, pk.bo, residual=x)                      # bf16
        y = ops.layernorm(y, pk.g1, pk.e1, _LN_EPS)                                   # bf16
        h = ops.gemm(y, pk.w1, pk.b1, epilogue=ops.EPI_RELU)                          # bf16
        z = ops.gemm(h, pk.w2, pk.b2, residual=y)                                     # bf16
        return ops.layernorm(z, pk.g2, pk.e2, _LN_EPS)                                # bf16

    def forward(self, src, src_mask=None, src_key_padding_mask=None, pos=None):
        """The reference's contract: src / pos [N, bs, C]; src_mask bool [bs, N, N] (or already [bs * nhead, N, N]) with True = NOT allowed, as
        nn.MultiheadAttention reads it; src_key_padding_mask is accepted and unused, as in the reference (:115-117).  Returns [N, bs, C]."""
        require_inference(self, (self.dropout_rate,))
        if src_mask is None:
            raise ValueError("TransformerEncoderLayer: src_mask is required (the reference dereferences it unconditionally, :109)")
        N, B, C = src.shape
        allowed = ~src_mask.to(device=src.device, dtype=torch.bool)
        if allowed.dim() == 3 and allowed.shape[0] == B:
            mask = expand_text_mask(allowed, self.nhead)
        elif allowed.dim() == 3 and allowed.shape[0] == B * self.nhead:
            mask = allowed.contiguous().view(torch.uint8)
        else:
            raise ValueError(f"TransformerEncoderLayer: src_mask of shape {tuple(src_mask.shape)}; expected [{B}, {N}, {N}] or [{B * self.nhead}, {N}, {N}]")
        x = as_rows(src.transpose(0, 1))
        p = None if pos is None else as_rows(pos.transpose(0, 1))
        out = self.rows_forward(x, p, mask, B, N)
        return out.view(B, N, C).transpose(0, 1).to(src.dtype)
