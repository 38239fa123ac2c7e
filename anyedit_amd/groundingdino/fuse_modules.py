"""GroundingDINO/groundingdino/models/GroundingDINO/fuse_modules.py:99-295 — the image-text fusion of the feature enhancer on the HIP path.

`BiAttentionBlock` restated over the library, both token streams as bf16 rows:

    vn = layer_norm_v(v), ln = layer_norm_l(l)                                         ops.layernorm
    q | val_v = vn [v_proj ; values_v_proj]^T,  k | val_l = ln [l_proj ; values_l_proj]^T   ONE ops.gemm per stream (+bias), [rows, 2 embed_dim]
    out_v, out_l = the two softmaxes over ONE logit matrix                              ops.bi_attention (csrc/gdino_encoder.hip), reads the
                                                                                        halves of the packed rows through their row stride
    v' = vn + gamma_v (out_v out_v_proj^T + b),  l' = ln + gamma_l (...)                ops.gemm (fp32 product) + ops.scale_residual

The residual is the reference's: `v = self.layer_norm_v(v)` rebinds `v` (:287), so the block returns LN(v) + gamma_v delta_v, not v_in + ...
Every activation stored between two launches is bf16 (the points are marked `# bf16:`; tests/gdino_enc_ref.py rounds at exactly those points for its
control); the out-projection products stay fp32 until the residual is formed.  Inference only.
"""
import types

import torch
import torch.nn as nn

from anyedit_amd import ops

BF16 = torch.bfloat16
_LN_EPS = 1e-5


def _f32(t):
    return t.detach().float().contiguous()


def require_inference(mod, dropouts=()):
    """The enhancer has no backward and no dropout kernels: refuse what would silently need them."""
    if mod.training and any(float(p) > 0.0 for p in dropouts):
        raise RuntimeError(f"{type(mod).__name__}: forward in train() mode with a non-zero dropout is not built (inference only): call .eval()")
    if torch.is_grad_enabled() and any(p.requires_grad for p in mod.parameters()):
        raise RuntimeError(f"{type(mod).__name__}: inference only: there is no backward for this path; call it under torch.no_grad() "
                           "or set requires_grad_(False) on its parameters")


def as_rows(x):
    """[B, N, C] of any float dtype -> contiguous bf16 rows [B*N, C]."""
    B, N, C = x.shape
    return x.detach().to(BF16).contiguous().view(B * N, C)


def _mask_u8(mask, B, N, device):
    if mask is None:
        return None
    if tuple(mask.shape) != (B, N):
        raise ValueError(f"attention mask of shape {tuple(mask.shape)}; expected {(B, N)}")
    return mask.to(device=device, dtype=torch.bool).contiguous().view(torch.uint8)


class BiMultiHeadAttention(nn.Module):
    """:99-248.  `forward(v, l, attention_mask_v, attention_mask_l)` returns (delta_v, delta_l) in the input's dtype.  The masks are the
    reference's: True = a padded token.  The global-maximum subtraction (:181-182) and the clamps to +-50000 (:184-202) are left out: they
    change a result only when the logits of one call span more than 50000 (include/anyedit_hip.h, ae_biattn_bf16)."""

    def __init__(self, v_dim, l_dim, embed_dim, num_heads, dropout=0.1, cfg=None):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.v_dim, self.l_dim = v_dim, l_dim
        if self.head_dim * num_heads != embed_dim:
            raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {embed_dim} and `num_heads`: {num_heads}).")
        if self.head_dim != ops.BIATTN_HEAD_DIM:
            raise ValueError(f"BiMultiHeadAttention: head_dim {embed_dim}/{num_heads} = {self.head_dim}; ae_biattn_bf16 is built for head_dim "
                             f"{ops.BIATTN_HEAD_DIM} only (GroundingDINO: embed_dim 1024, 4 heads)")
        if v_dim % 8 or l_dim % 8:
            raise ValueError(f"BiMultiHeadAttention: v_dim {v_dim} and l_dim {l_dim} must be multiples of 8")
        self.scale = self.head_dim ** (-0.5)
        self.dropout = dropout
        self.v_proj = nn.Linear(v_dim, embed_dim)
        self.l_proj = nn.Linear(l_dim, embed_dim)
        self.values_v_proj = nn.Linear(v_dim, embed_dim)
        self.values_l_proj = nn.Linear(l_dim, embed_dim)
        self.out_v_proj = nn.Linear(embed_dim, v_dim)
        self.out_l_proj = nn.Linear(embed_dim, l_dim)
        self.stable_softmax_2d = True
        self.clamp_min_for_underflow = True
        self.clamp_max_for_overflow = True
        self._reset_parameters()

    def _reset_parameters(self):
        for m in (self.v_proj, self.l_proj, self.values_v_proj, self.values_l_proj, self.out_v_proj, self.out_l_proj):
            nn.init.xavier_uniform_(m.weight)
            m.bias.data.fill_(0)

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            cat = lambda a, b: ops.pack_linear(torch.cat([a.weight.detach(), b.weight.detach()], 0))
            catb = lambda a, b: torch.cat([_f32(a.bias), _f32(b.bias)], 0).contiguous()
            self._pk = types.SimpleNamespace(wv=cat(self.v_proj, self.values_v_proj), bv=catb(self.v_proj, self.values_v_proj),
                                             wl=cat(self.l_proj, self.values_l_proj), bl=catb(self.l_proj, self.values_l_proj),
                                             wov=ops.pack_linear(self.out_v_proj.weight), bov=_f32(self.out_v_proj.bias),
                                             wol=ops.pack_linear(self.out_l_proj.weight), bol=_f32(self.out_l_proj.bias))
        return self._pk

    def rows_forward(self, vn, ln, B, Nv, Nt, mask_v, mask_l):
        """vn [B*Nv, v_dim], ln [B*Nt, l_dim] bf16 rows, masks uint8 or None -> the fp32 products out_v out_v_proj^T [B*Nv, v_dim] and
        out_l out_l_proj^T [B*Nt, l_dim] WITHOUT their biases (`packed().bov / bol`; the caller's residual launch adds them)."""
        pk, E = self.packed(), self.embed_dim
        qv = ops.gemm(vn, pk.wv, pk.bv).view(B, Nv, 2 * E)            # bf16: q | val_v
        kl = ops.gemm(ln, pk.wl, pk.bl).view(B, Nt, 2 * E)            # bf16: k | val_l
        out_v, out_l = ops.bi_attention(qv[..., :E], kl[..., :E], qv[..., E:], kl[..., E:], self.num_heads, self.scale, mask_v, mask_l)   # bf16
        dv = ops.gemm(out_v.view(B * Nv, E), pk.wov, out_f32=True)
        dl = ops.gemm(out_l.view(B * Nt, E), pk.wol, out_f32=True)
        return dv, dl

    def forward(self, v, l, attention_mask_v=None, attention_mask_l=None):
        require_inference(self, (self.dropout,))
        B, Nv, _ = v.shape
        Nt = l.shape[1]
        vb, lb = as_rows(v), as_rows(l)
        dv, dl = self.rows_forward(vb, lb, B, Nv, Nt, _mask_u8(attention_mask_v, B, Nv, vb.device), _mask_u8(attention_mask_l, B, Nt, vb.device))
        pk = self.packed()
        return (dv + pk.bov).view(B, Nv, -1).to(v.dtype), (dl + pk.bol).view(B, Nt, -1).to(l.dtype)


class BiAttentionBlock(nn.Module):
    """:252-295.  `drop_path` is accepted: DropPath is the identity in eval(), and a non-zero rate in train() mode is refused like any dropout."""

    def __init__(self, v_dim, l_dim, embed_dim, num_heads, dropout=0.1, drop_path=0.0, init_values=1e-4, cfg=None):
        super().__init__()
        self.layer_norm_v = nn.LayerNorm(v_dim)
        self.layer_norm_l = nn.LayerNorm(l_dim)
        self.attn = BiMultiHeadAttention(v_dim=v_dim, l_dim=l_dim, embed_dim=embed_dim, num_heads=num_heads, dropout=dropout)
        self.drop_path_rate = drop_path
        self.gamma_v = nn.Parameter(init_values * torch.ones((v_dim)), requires_grad=True)
        self.gamma_l = nn.Parameter(init_values * torch.ones((l_dim)), requires_grad=True)

    def packed(self):
        ps = (self.layer_norm_v.weight, self.layer_norm_v.bias, self.layer_norm_l.weight, self.layer_norm_l.bias, self.gamma_v, self.gamma_l)
        if ops.cache_stale(self, "_pk", *ps):
            self._pk = types.SimpleNamespace(gv=_f32(ps[0]), ev=_f32(ps[1]), gl=_f32(ps[2]), el=_f32(ps[3]), gamma_v=_f32(ps[4]), gamma_l=_f32(ps[5]))
        return self._pk

    def rows_forward(self, x, t, B, Nv, Nt, mask_v, mask_l):
        """bf16 rows in, bf16 rows out: (LN(v) + gamma_v delta_v, LN(l) + gamma_l delta_l)."""
        pk, a = self.packed(), self.attn.packed()
        vn = ops.layernorm(x, pk.gv, pk.ev, _LN_EPS)                  # bf16: the v the reference rebinds (:287)
        ln = ops.layernorm(t, pk.gl, pk.el, _LN_EPS)                  # bf16
        dv, dl = self.attn.rows_forward(vn, ln, B, Nv, Nt, mask_v, mask_l)
        x = ops.scale_residual(dv, vn, pk.gamma_v, a.bov)             # bf16: :293
        t = ops.scale_residual(dl, ln, pk.gamma_l, a.bol)             # bf16: :294
        return x, t

    def forward(self, v, l, attention_mask_v=None, attention_mask_l=None):
        require_inference(self, (self.attn.dropout, self.drop_path_rate))
        B, Nv, _ = v.shape
        Nt = l.shape[1]
        x, t = as_rows(v), as_rows(l)
        x, t = self.rows_forward(x, t, B, Nv, Nt, _mask_u8(attention_mask_v, B, Nv, x.device), _mask_u8(attention_mask_l, B, Nt, x.device))
        return x.view(B, Nv, -1).to(v.dtype), t.view(B, Nt, -1).to(l.dtype)
