"""GroundingDINO/groundingdino/models/GroundingDINO/backbone/swin_transformer.py — the detector's image backbone on the HIP path: the Swin
Transformer that turns the 800-pixel image of tools/tool.py:91-102 into the multi-scale maps GroundingDINO's feature enhancer reads
(`GroundingDINO.backbone[0]`, built by `build_swin_transformer` from `GroundingDINO_SwinB_cfg.py` / `GroundingDINO_SwinT_OGC.py`).

The tower restated over the library, rows in IMAGE order [B*H*W, C] from the patch embedding to the outputs:

    pixels (right / bottom zero pad to a multiple of 4) -> patch rows (im2col) -> patch GEMM + conv bias -> patch norm                = x of stage 0
    per stage, depth blocks, each
        h = norm1(x) -> q|k|v (ONE [3C, C] GEMM, +bias) -> shifted-window attention (ONE launch, below) -> proj (+bias), +x           = x'
        h = norm2(x') -> fc1 (fp32 product) -> +bias, GELU -> fc2 (+bias), +x'                                                        = next x
      norm{i} of every row -> NCHW                                                                                                    = output i
      PatchMerging: 2x2 gather + LayerNorm over 4C (ONE launch) -> reduction GEMM                                                     = x of the next stage

Every operator of a block except the attention is per token, so the reference's pad / roll / window_partition / window_reverse / roll back /
crop (:253-292) only decide which tokens attend to each other: they are the row addressing of `ops.swin_window_attention`
(csrc/swin.hip), which reads q | k | v at image rows and writes the result to image rows; no padded, rolled or partitioned copy of the
activation exists.  Pad tokens take part in the softmax with key = value = the qkv bias (the reference pads AFTER norm1, then applies qkv), the
-100 shift mask of BasicLayer.forward (:417-443) is computed in the kernel, and the relative position bias is gathered to [nH, N, N] when a
block's weights are packed (re-made when the table changes).  Kernels: `ops.clip_patch_rows`, `ops.gemm`, `ops.layernorm`,
`ops.swin_window_attention`, `ops.bias_act`, `ops.swin_merge_layernorm`, `ops.rows_to_nchw_out`.  Every activation stored between two launches
is bf16; the points are marked `# bf16:` below and tests/swin_ref.py rounds at exactly those points for its control.

Parameters and buffers carry the reference's names (`patch_embed.{proj, norm}`, `layers.I.blocks.J.{norm1, attn.{qkv, proj,
relative_position_bias_table, relative_position_index}, norm2, mlp.{fc1, fc2}}`, `layers.I.downsample.{norm, reduction}`, `normI`), so the
`backbone.0.*` entries of a GroundingDINO checkpoint fill the tower (`checkpoints.load_groundingdino_backbone`).  The persistent
`relative_position_index` buffer loads and is checked against the computed one.

One call on a given (B, H, W, dtype) makes no allocation and no host synchronisation after the first with the same arguments, runs on the
current stream only and may be captured in a graph: its buffers (the returned maps included) are static per shape.
"""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from anyedit_amd import ops
from anyedit_amd.groundingdino.misc import NestedTensor

BF16 = torch.bfloat16
_LN_EPS = 1e-5                                   # nn.LayerNorm's default: the reference never passes another
_LN_CMAX = 4096                                  # ae_layernorm_bf16: the widest row of norm1 / norm2 / norm{i}

# build_swin_transformer's table (:771-787)
SWIN_GEOMETRIES = {
    "swin_T_224_1k": dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7),
    "swin_B_224_22k": dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=7),
    "swin_B_384_22k": dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=12),
    "swin_L_224_22k": dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48], window_size=7),
    "swin_L_384_22k": dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48], window_size=12),
}


def relative_position_index(window_size):
    """:113-123: [N, N] int64, entry (a, b) = (ya - yb + ws - 1) * (2 ws - 1) + (xa - xb + ws - 1) for window positions a, b in row-major order."""
    ws = window_size
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    return (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)


def _f32(t):
    return t.detach().float().contiguous()


class PatchEmbed(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim, patch_norm):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim) if patch_norm else None


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads, qkv_bias, qk_scale):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", relative_position_index(window_size))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + "relative_position_index"
        if key in state_dict:
            want = relative_position_index(self.window_size)
            got = state_dict[key]
            if tuple(got.shape) != tuple(want.shape) or not torch.equal(got.detach().cpu().long(), want):
                error_msgs.append(f"{key}: the stored buffer is not the relative position index of a {self.window_size}x{self.window_size} window "
                                  "(the bias gather would read other table rows than the checkpoint was trained with)")
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def gathered_bias(self):
        """:151-158: relative_position_bias_table[relative_position_index] as fp32 [nH, N, N]."""
        N = self.window_size ** 2
        t = self.relative_position_bias_table.detach().float()
        return t[self.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(dim, hidden), nn.Linear(hidden, dim)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, shift_size, mlp_ratio, qkv_bias, qk_scale):
        super().__init__()
        self.window_size, self.shift_size = window_size, shift_size
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, window_size, num_heads, qkv_bias, qk_scale)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def packed(self):
        """bf16 weight images, fp32 biases / affine vectors and the gathered relative position bias of this block; rebuilt when any of its
        tensors changes (the bias follows relative_position_bias_table)."""
        if ops.cache_stale(self, "_pk", *self.parameters()):
            a, m = self.attn, self.mlp
            C = a.dim
            bqkv = _f32(a.qkv.bias) if a.qkv.bias is not None else torch.zeros(3 * C, dtype=torch.float32, device=a.qkv.weight.device)
            self._pk = types.SimpleNamespace(wqkv=ops.pack_linear(a.qkv.weight), bqkv=bqkv, rpb=a.gathered_bias(), wo=ops.pack_linear(a.proj.weight),
                                             bo=_f32(a.proj.bias), w1=ops.pack_linear(m.fc1.weight), b1=_f32(m.fc1.bias), w2=ops.pack_linear(m.fc2.weight),
                                             b2=_f32(m.fc2.bias), g1=_f32(self.norm1.weight), e1=_f32(self.norm1.bias), g2=_f32(self.norm2.weight),
                                             e2=_f32(self.norm2.bias))
        return self._pk


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            self._pk = types.SimpleNamespace(w=ops.pack_linear(self.reduction.weight), g=_f32(self.norm.weight), e=_f32(self.norm.bias))
        return self._pk


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale, downsample):
        super().__init__()
        self.dim, self.num_heads, self.window_size = dim, num_heads, window_size
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio, qkv_bias, qk_scale)
                                     for i in range(depth)])        # :390: every odd block shifts, whatever the size of the map
        self.downsample = PatchMerging(dim) if downsample else None


class SwinTransformer(nn.Module):
    """swin_transformer.py:501-759 on HIP, the reference's constructor arguments.  `drop_rate`, `attn_drop_rate`, `drop_path_rate`,
    `use_checkpoint` and `frozen_stages` are accepted and change nothing at inference; `norm_layer` must be nn.LayerNorm; `ape=True` is refused.
    `dilation=True` changes which stages downsample, as in the reference (:599-604); it also halves the last stage's width, so with a head count
    of build_swin_transformer's table that stage has head_dim 16 and is refused like any head_dim other than 32 (backbone.py:203 never sets it)."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2, norm_layer=nn.LayerNorm, ape=False,
                 patch_norm=True, out_indices=(0, 1, 2, 3), frozen_stages=-1, dilation=False, use_checkpoint=False):
        super().__init__()
        if ape:
            raise ValueError("SwinTransformer: ape=True (an absolute position embedding) is not built: no GroundingDINO config sets it")
        if norm_layer is not nn.LayerNorm:
            raise ValueError("SwinTransformer: norm_layer must be nn.LayerNorm (the only one the reference's configs use)")
        if isinstance(patch_size, (tuple, list)):
            if patch_size[0] != patch_size[1]:
                raise ValueError(f"SwinTransformer: square patches only, got {tuple(patch_size)}")
            patch_size = patch_size[0]
        depths, num_heads = list(depths), list(num_heads)
        if len(depths) != len(num_heads) or not depths:
            raise ValueError(f"SwinTransformer: depths {depths} and num_heads {num_heads} must name the same stages")
        if not 1 <= window_size <= ops.SWIN_MAX_WINDOW:
            raise ValueError(f"SwinTransformer: window_size {window_size} must be in [1, {ops.SWIN_MAX_WINDOW}] (ae_swin_window_attn_bf16 keeps a whole window's keys resident)")
        L = len(depths)
        num_features = [int(embed_dim * 2 ** i) for i in range(L)]
        downsample = [i < L - 1 for i in range(L)]
        if dilation:                               # :602-604: the last stage keeps the resolution and the width of the one before it
            if L < 2:
                raise ValueError("SwinTransformer: dilation=True needs at least two stages")
            downsample[-2] = False
            num_features[-1] = int(embed_dim * 2 ** (L - 1)) // 2
        for i, (C, nH) in enumerate(zip(num_features, num_heads)):
            if nH <= 0 or C % nH or C // nH != ops.SWIN_HEAD_DIM:
                raise ValueError(f"SwinTransformer: stage {i} has head_dim {C}/{nH}; ae_swin_window_attn_bf16 is built for head_dim {ops.SWIN_HEAD_DIM} only "
                                 "(every geometry of build_swin_transformer has it)")
            if int(C * mlp_ratio) % 8 or C % 8 or C > _LN_CMAX:
                raise ValueError(f"SwinTransformer: stage {i}: width {C} and hidden width {int(C * mlp_ratio)} must be multiples of 8, the width at most {_LN_CMAX}")
            if downsample[i] and C > ops.SWIN_MERGE_CMAX:          # only a stage that merges has a LayerNorm over 4C
                raise ValueError(f"SwinTransformer: stage {i} merges patches at width {C}; ae_swin_merge_ln_bf16 normalises at most 4 * {ops.SWIN_MERGE_CMAX} values")
        out_indices = tuple(out_indices)
        if any(i < 0 or i >= L for i in out_indices):
            raise ValueError(f"SwinTransformer: out_indices {out_indices} are outside [0, {L})")
        self.pretrain_img_size, self.num_layers, self.embed_dim, self.ape, self.patch_norm = pretrain_img_size, L, embed_dim, False, patch_norm
        self.out_indices, self.frozen_stages, self.dilation = out_indices, frozen_stages, dilation
        self.patch_size, self.in_chans, self.window_size, self.mlp_ratio = patch_size, in_chans, window_size, mlp_ratio
        self.num_features = num_features
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim, patch_norm)
        self.layers = nn.ModuleList([BasicLayer(num_features[i], depths[i], num_heads[i], window_size, mlp_ratio, qkv_bias, qk_scale, downsample[i])
                                     for i in range(L)])
        for i in out_indices:
            self.add_module(f"norm{i}", nn.LayerNorm(num_features[i]))
        self._ws = {}
        self._freeze_stages()

    def _freeze_stages(self):                      # :636-651
        if self.frozen_stages >= 0:
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 2:
            for i in range(0, self.frozen_stages - 1):
                for p in self.layers[i].parameters():
                    p.requires_grad = False

    def train(self, mode=True):
        """:756-759 (whose override returns None; this one returns self, as nn.Module.train does)."""
        super().train(mode)
        self._freeze_stages()
        return self

    @property
    def device(self):
        return self.patch_embed.proj.weight.device

    def weights_token(self):
        """Changes whenever any parameter of the tower does (callers cache encodings against it)."""
        return ops.weights_token(*self.parameters())

    # ---- caches ---------------------------------------------------------------------------------------------------------------
    def _tables(self):
        pe = self.patch_embed
        norms = [getattr(self, f"norm{i}") for i in self.out_indices]
        ps = [pe.proj.weight, pe.proj.bias] + ([pe.norm.weight, pe.norm.bias] if pe.norm is not None else []) + [t for n in norms for t in (n.weight, n.bias)]
        if ops.cache_stale(self, "_pk", *ps):
            self._pk = types.SimpleNamespace(wpatch=ops.pack_patch_embedding(pe.proj.weight), bpatch=_f32(pe.proj.bias),
                                             gp=_f32(pe.norm.weight) if pe.norm is not None else None, ep=_f32(pe.norm.bias) if pe.norm is not None else None,
                                             norm={i: (_f32(n.weight), _f32(n.bias)) for i, n in zip(self.out_indices, norms)})
        return self._pk

    def stage_sizes(self, H, W):
        """[(H_i, W_i)] of the token map of every stage for an H x W image."""
        P = self.patch_size
        h, w = (H + P - 1) // P, (W + P - 1) // P
        out = []
        for layer in self.layers:
            out.append((h, w))
            if layer.downsample is not None:
                h, w = (h + 1) // 2, (w + 1) // 2
        return out

    def _workspace(self, B, H, W, dtype, dev):
        key = (B, H, W, dtype, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            P, Cin = self.patch_size, self.in_chans
            Hc, Wc = (H + P - 1) // P * P, (W + P - 1) // P * P
            e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
            sizes = self.stage_sizes(H, W)
            stages = []
            for (h, w), layer in zip(sizes, self.layers):
                M, C = B * h * w, layer.dim
                Hd = int(C * self.mlp_ratio)
                st = types.SimpleNamespace(H=h, W=w, M=M, C=C, x0=e(M, C), xa=e(M, C), xb=e(M, C), h=e(M, C), qkv=e(M, 3 * C), att=e(M, C), mid=e(M, C),
                                           u=e(M, Hd, dt=torch.float32), act=e(M, Hd), z=e(M, C), out=e(B, C, h, w, dt=dtype), merged=None)
                if layer.downsample is not None:
                    st.merged = e(B * ((h + 1) // 2) * ((w + 1) // 2), 4 * C)
                stages.append(st)
            h0, w0 = sizes[0]
            ws = self._ws[key] = types.SimpleNamespace(
                px=torch.zeros(B, Cin, Hc, Wc, dtype=dtype, device=dev) if (Hc, Wc) != (H, W) else None,      # :486-489: right / bottom zero padding, the zeros written once
                rows=e(B * h0 * w0, ops.clip_patch_kpad(Cin, P)), emb=e(B * h0 * w0, self.embed_dim), stages=stages)
        return ws

    # ---- the tower ------------------------------------------------------------------------------------------------------------
    def _pixels(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.in_chans or x.shape[0] < 1:
            raise ValueError(f"SwinTransformer: expected a [B, {self.in_chans}, H, W] tensor")
        if x.dtype not in (torch.float32, BF16):
            raise TypeError(f"SwinTransformer: expected fp32 or bf16 pixels, got {x.dtype}")
        if self.device.type != "cuda" or not x.is_cuda:
            raise ValueError("SwinTransformer: the tower runs on the GPU only (anyedit_amd has no CPU path); move the tower and the pixels with .to('cuda')")
        if not x.is_contiguous():
            raise ValueError("SwinTransformer: expected a contiguous tensor (a copy would be an allocation inside the forward)")
        B, _, H, W = x.shape
        if H < 1 or W < 1:
            raise ValueError(f"SwinTransformer: empty image {H}x{W}")
        ws = self._workspace(B, H, W, x.dtype, self.device)
        if ws.px is not None:
            ws.px[:, :, :H, :W].copy_(x)
            x = ws.px
        return x, ws

    @torch.no_grad()
    def run(self, x):
        """Runs the tower; returns the workspace of this (B, H, W, dtype): `ws.stages[i]` holds stage i's input rows `x0` [B*H_i*W_i, C_i] bf16, its
        size (H, W) and, for a stage of out_indices, the normed NCHW map `out` in the input's dtype."""
        px, ws = self._pixels(x)
        B = px.shape[0]
        t = self._tables()
        wsz = self.window_size
        s0 = ws.stages[0]
        ops.clip_patch_rows(px, self.patch_size, out=ws.rows)                                        # bf16: pixels as patch rows
        if t.gp is not None:
            ops.gemm(ws.rows, t.wpatch, t.bpatch, out=ws.emb)                                        # bf16: patch embedding
            ops.layernorm(ws.emb, t.gp, t.ep, _LN_EPS, out=s0.x0)                                    # bf16: patch norm output
        else:
            ops.gemm(ws.rows, t.wpatch, t.bpatch, out=s0.x0)                                         # bf16: patch embedding
        for i, layer in enumerate(self.layers):
            st = ws.stages[i]
            cur = st.x0                                                                              # x0 stays the stage's input; the stream alternates between xa and xb
            for k, blk in enumerate(layer.blocks):
                nxt = st.xb if k % 2 else st.xa
                p = blk.packed()
                ops.layernorm(cur, p.g1, p.e1, _LN_EPS, out=st.h)                                    # bf16: norm1 output
                ops.gemm(st.h, p.wqkv, p.bqkv, out=st.qkv)                                           # bf16: packed q | k | v
                ops.swin_window_attention(st.qkv, p.bqkv, p.rpb, B, st.H, st.W, layer.num_heads, wsz, blk.shift_size, blk.attn.scale, out=st.att)   # bf16: attention output
                ops.gemm(st.att, p.wo, p.bo, residual=cur, out=st.mid)                               # bf16: residual stream after the attention add
                ops.layernorm(st.mid, p.g2, p.e2, _LN_EPS, out=st.h)                                 # bf16: norm2 output
                ops.gemm(st.h, p.w1, None, out_f32=True, out=st.u)                                   # fp32: fc1 product (bias and GELU follow in fp32)
                ops.bias_act(st.u, p.b1, ops.ACT_GELU, out=st.act)                                   # bf16: activated hidden values
                ops.gemm(st.act, p.w2, p.b2, residual=st.mid, out=nxt)                               # bf16: residual stream after the MLP add
                cur = nxt
            if i in self.out_indices:
                g, e = t.norm[i]
                ops.layernorm(cur, g, e, _LN_EPS, out=st.z)                                          # bf16: output norm
                ops.rows_to_nchw_out(st.z, st.out)
            if layer.downsample is not None:
                d = layer.downsample.packed()
                ops.swin_merge_layernorm(cur, d.g, d.e, B, st.H, st.W, _LN_EPS, out=st.merged)       # bf16: merged and normed rows
                ops.gemm(st.merged, d.w, None, out=ws.stages[i + 1].x0)                              # bf16: reduced rows = the next stage's input
            elif i + 1 < self.num_layers:
                ws.stages[i + 1].x0.copy_(cur)                                                        # dilation: the next stage runs at this resolution and width
        return ws

    def forward_raw(self, x):
        """:678-710: the tuple of NCHW maps of out_indices, in the input's dtype.  Static buffers of this (B, H, W, dtype): valid until the next call
        of that shape."""
        ws = self.run(x)
        return tuple(ws.stages[i].out for i in range(self.num_layers) if i in self.out_indices)

    def forward(self, tensor_list):
        """:712-754: {idx: NestedTensor(map, mask)}, the padding mask nearest-interpolated to every map."""
        outs = self.forward_raw(tensor_list.tensors)
        m = tensor_list.mask
        if m is None:
            raise ValueError("SwinTransformer.forward: the NestedTensor carries no mask")
        return {idx: NestedTensor(o, F.interpolate(m[None].float(), size=o.shape[-2:]).to(torch.bool)[0]) for idx, o in enumerate(outs)}


def build_swin_transformer(modelname, pretrain_img_size, **kw):
    """:762-791: one of the reference's five geometries; `kw` overrides (dilation, out_indices, use_checkpoint, ...)."""
    if modelname not in SWIN_GEOMETRIES:
        raise ValueError(f"build_swin_transformer: unknown model {modelname!r} (known: {sorted(SWIN_GEOMETRIES)})")
    cfg = {k: (list(v) if isinstance(v, list) else v) for k, v in SWIN_GEOMETRIES[modelname].items()}
    cfg.update(kw)
    return SwinTransformer(pretrain_img_size=pretrain_img_size, **cfg)
