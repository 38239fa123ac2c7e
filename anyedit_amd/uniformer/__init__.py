"""UniFormer backbone on HIP: mirror of AnyEdit_Collection/other_modules/uniformer/mmseg/models/backbones/uniformer.py, the backbone of the
`visual_segment` condition's annotator (`img2seg`: UniFormer-S + UPerNet, seg_config.py).  Same class names, constructor keywords, parameter
names and state-dict keys (the BatchNorm buffers included), so the `backbone.*` entries of an mmseg checkpoint load strictly
(checkpoints.load_uniformer).  Inference only (eval mode: drop-path and dropout are identities, BatchNorm uses its running statistics).

Launches of one `forward` at the UniFormer-S geometry (layers 3 / 4 / 8 / 3, widths 64 / 128 / 320 / 512, head dim 64): 146 at 512x512.  ops.ln_gemm
decides per shape whether the LayerNorm runs inside the projection's launch; at this geometry's shapes (M = 1024, K = 320 and M = 256, K = 512) the
library's fused kernel covers none, so a LayerNorm launch stands in front of both projections of every SABlock (8 launches each; 6 where it folds):
    PatchEmbed (4 x)   ops.clip_patch_rows (stage 1, 4x4 from the pixels) or ops.patch2_rows (2x2 from the rows); ops.gemm + bias;
                       ops.layernorm (eps 1e-5)                                                                                       3 each
    CBlock (3 + 4 x)   ops.dwconv k = 3, residual = x            x + pos_embed(x)
                       ops.gemm                                  conv1 with BatchNorm norm1 folded into its weight and bias
                       ops.dwconv k = 5                          attn
                       ops.gemm + residual                       x + conv2(.)
                       ops.gemm, EPI_GELU                        mlp.fc1 with BatchNorm norm2 folded in, GELU
                       ops.gemm + residual                       x + mlp.fc2(.)                                                       6 each
    SABlock (8 + 3 x)  ops.dwconv k = 3, residual = x            x + pos_embed(x)
                       ops.ln_gemm                               norm1 + attn.qkv
                       ops.attention                             global, dim // 64 heads, on the packed q | k | v rows
                       ops.gemm + residual                       x + attn.proj(.)
                       ops.ln_gemm, EPI_GELU                     norm2 + mlp.fc1, GELU
                       ops.gemm + residual                       x + mlp.fc2(.)                                                       6 or 8 each
    outputs (4 x)      ops.layernorm_rows_nchw                   norm_i over channels, fp32 [B, C, H, W] (and the bf16 rows)            1 each
Activations between launches are bf16 channels-last rows [B*H*W, C]; the depthwise weights, every bias and every LayerNorm parameter are fp32;
the matrices are bf16 (the BatchNorm folds are done in fp32 before that rounding).  No host synchronisation: `forward` is capturable in a graph.

Not built: `windows=True` (SABlock_Windows :168-215), `hybrid=True`, `use_checkpoint`, `representation_size`; the UPerNet head, the ADE palette
and `img2seg` itself.
"""
import types
from functools import partial

import torch
from torch import nn

from anyedit_amd import ops

MIN_SIDE = 32      # below it the stride-32 map is empty


def fold_bn(weight, bias, gamma, beta, mean, var, eps):
    """A BatchNorm in eval mode directly in front of a 1x1 convolution / Linear: W (s x + t) + b = (W s) x + (W t + b) with s = gamma / sqrt(var +
    eps), t = beta - mean s.  weight [N, K(, 1, 1)]; returns ([N, K], [N]) in the dtype of the arguments (the module folds in fp32)."""
    w = weight.reshape(weight.shape[0], -1)
    s = gamma / torch.sqrt(var + eps)
    t = beta - mean * s
    return w * s.unsqueeze(0), bias + w @ t


def _f32(t):
    return t.detach().float().contiguous()


class Mlp(nn.Module):
    """:24-40"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _only_gelu(act_layer)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)


class CMlp(nn.Module):
    """:43-59"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _only_gelu(act_layer)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Conv2d(in_features, hidden_features, 1)
        self.fc2 = nn.Conv2d(hidden_features, out_features, 1)


def _only_gelu(act_layer):
    if act_layer is not nn.GELU:
        raise NotImplementedError(f"uniformer: act_layer={act_layer} is not built: the fused epilogue is the exact-erf GELU")


def _check_dim(what, dim):
    if dim % 8 or dim < 8:
        raise ValueError(f"{what}: dim={dim} must be a multiple of 8 (the kernels take 8 channels, 16 bytes, per lane)")


class CBlock(nn.Module):
    """:62-81.  `rows` is the launch chain on bf16 rows [B*H*W, dim]."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        _check_dim("CBlock", dim)
        self.pos_embed = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.norm1 = nn.BatchNorm2d(dim)
        self.conv1 = nn.Conv2d(dim, dim, 1)
        self.conv2 = nn.Conv2d(dim, dim, 1)
        self.attn = nn.Conv2d(dim, dim, 5, padding=2, groups=dim)
        self.norm2 = nn.BatchNorm2d(dim)
        self.mlp = CMlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def _tensors(self):
        bn = lambda n: [n.weight, n.bias, n.running_mean, n.running_var]
        return list(self.parameters()) + bn(self.norm1) + bn(self.norm2)

    def packed(self):
        """Packed weights, rebuilt when a parameter or a BatchNorm buffer changes: fp32 tap-major depthwise images, bf16 matrices with the
        BatchNorms folded in fp32 before the rounding, fp32 biases."""
        if ops.cache_stale(self, "_pk", *self._tensors()):
            def folded(conv, bn):
                w, b = fold_bn(conv.weight.detach().float(), conv.bias.detach().float(), bn.weight.detach().float(), bn.bias.detach().float(),
                               bn.running_mean.detach().float(), bn.running_var.detach().float(), bn.eps)
                return ops.pack_linear(w), b.contiguous()
            self._pk = types.SimpleNamespace(
                dw3=(ops.pack_dwconv(self.pos_embed.weight), _f32(self.pos_embed.bias)), dw5=(ops.pack_dwconv(self.attn.weight), _f32(self.attn.bias)),
                conv1=folded(self.conv1, self.norm1), conv2=(ops.pack_linear(self.conv2.weight), _f32(self.conv2.bias)),
                fc1=folded(self.mlp.fc1, self.norm2), fc2=(ops.pack_linear(self.mlp.fc2.weight), _f32(self.mlp.fc2.bias)))
        return self._pk

    def rows(self, x, B, H, W):
        pk = self.packed()
        x = ops.dwconv(x, *pk.dw3, B, H, W, residual=x)                    # bf16: x + pos_embed(x)
        t = ops.gemm(x, *pk.conv1)                                         # bf16: conv1(norm1(x))
        t = ops.dwconv(t, *pk.dw5, B, H, W)                                # bf16: attn(.)
        x = ops.gemm(t, *pk.conv2, residual=x)                             # bf16: x + conv2(.)
        t = ops.gemm(x, *pk.fc1, epilogue=ops.EPI_GELU)                    # bf16: GELU(fc1(norm2(x)))
        return ops.gemm(t, *pk.fc2, residual=x)                            # bf16: x + fc2(.)


class Attention(nn.Module):
    """:84-109"""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        if num_heads < 1 or dim % num_heads:
            raise ValueError(f"Attention: dim={dim} is not a whole number of {num_heads} heads")
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class SABlock(nn.Module):
    """:112-135.  `rows` is the launch chain on bf16 rows [B*H*W, dim]; the attention is global over the H*W tokens of each image."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        _check_dim("SABlock", dim)
        self.pos_embed = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            lin = lambda m: (ops.pack_linear(m.weight), None if m.bias is None else _f32(m.bias))
            self._pk = types.SimpleNamespace(
                dw3=(ops.pack_dwconv(self.pos_embed.weight), _f32(self.pos_embed.bias)), ln1=(_f32(self.norm1.weight), _f32(self.norm1.bias), self.norm1.eps),
                ln2=(_f32(self.norm2.weight), _f32(self.norm2.bias), self.norm2.eps), qkv=lin(self.attn.qkv), proj=lin(self.attn.proj), fc1=lin(self.mlp.fc1),
                fc2=lin(self.mlp.fc2))
        return self._pk

    def rows(self, x, B, H, W):
        pk = self.packed()
        N, C, heads = H * W, x.shape[1], self.attn.num_heads
        D = C // heads
        x = ops.dwconv(x, *pk.dw3, B, H, W, residual=x)                    # bf16: x + pos_embed(x)
        qkv = ops.ln_gemm(x, *pk.ln1, *pk.qkv)                             # bf16: qkv(norm1(x)), packed q | k | v
        st = (N * 3 * C, D, 3 * C)
        a = ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], B, heads, N, N, D, float(self.attn.scale), st, st, st)     # bf16 [B, N, C]
        x = ops.gemm(a.view(B * N, C), *pk.proj, residual=x)               # bf16: x + proj(.)
        t = ops.ln_gemm(x, *pk.ln2, *pk.fc1, epilogue=ops.EPI_GELU)        # bf16: GELU(fc1(norm2(x)))
        return ops.gemm(t, *pk.fc2, residual=x)                            # bf16: x + fc2(.)


class PatchEmbed(nn.Module):
    """:218-239: Conv2d(kernel = stride = patch) then nn.LayerNorm(embed_dim) with its default eps (1e-5, not the blocks' 1e-6).  Built: patch 4
    from the fp32 pixels (`from_pixels`) and patch 2 from bf16 rows (`from_rows`); a map that is not a whole number of patches loses its last rows /
    columns, as the strided convolution drops them."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        two = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        img_size, patch_size = two(img_size), two(patch_size)
        if patch_size[0] != patch_size[1] or patch_size[0] < 1:
            raise NotImplementedError(f"PatchEmbed: square patches only, got {patch_size}")
        _check_dim("PatchEmbed", embed_dim)
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0])
        self.norm = nn.LayerNorm(embed_dim)
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

    def packed(self, from_pixels):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            w = ops.pack_patch_embedding(self.proj.weight.detach().float()) if from_pixels else ops.pack_patch2(self.proj.weight.detach().float())
            self._pk = types.SimpleNamespace(w=w, b=_f32(self.proj.bias), g=_f32(self.norm.weight), beta=_f32(self.norm.bias), eps=self.norm.eps)
        return self._pk

    def _project(self, rows, pk):
        return ops.layernorm(ops.gemm(rows, pk.w, pk.b), pk.g, pk.beta, pk.eps)        # bf16: proj, then bf16: norm

    def from_pixels(self, x):
        """x fp32 [B, Cin, H, W] -> (rows, H // p, W // p)"""
        p = self.patch_size[0]
        B, _, H, W = x.shape
        h, w = H // p, W // p
        if H % p or W % p:
            x = x[:, :, :h * p, :w * p]
        return self._project(ops.clip_patch_rows(x.contiguous(), p), self.packed(True)), h, w

    def from_rows(self, x, B, H, W):
        if self.patch_size[0] != 2:
            raise NotImplementedError(f"PatchEmbed: from rows only the 2x2 patch is built, got {self.patch_size}")
        rows, h, w = ops.patch2_rows(x, B, H, W)
        return self._project(rows, self.packed(False)), h, w


class UniFormer(nn.Module):
    """:243-422 with the reference's keywords.  `forward(x)`: fp32 [B, 3, H, W] normalised pixels on the GPU -> the tuple of four fp32 NCHW maps at
    strides 4, 8, 16, 32; `forward_rows(x)`: the same four outputs as bf16 rows, [(rows [B*h*w, C], h, w), ...].  The dropout rates are accepted
    and ignored (inference only); `pretrained_path` goes through checkpoints.load_uniformer."""

    def __init__(self, layers=[3, 4, 8, 3], img_size=224, in_chans=3, num_classes=80, embed_dim=[64, 128, 320, 512], head_dim=64, mlp_ratio=4.,
                 qkv_bias=True, qk_scale=None, representation_size=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer=partial(nn.LayerNorm, eps=1e-6), pretrained_path=None, use_checkpoint=False, checkpoint_num=[0, 0, 0, 0], windows=False,
                 hybrid=False, window_size=14):
        super().__init__()
        if windows:
            raise NotImplementedError("UniFormer: windows=True (SABlock_Windows, local window attention in stage 3) is not built")
        if hybrid:
            raise NotImplementedError("UniFormer: hybrid=True (window and global blocks mixed in stage 3) is not built")
        if use_checkpoint:
            raise NotImplementedError("UniFormer: use_checkpoint=True (activation checkpointing) is not built: this backbone is inference only")
        if representation_size:
            raise NotImplementedError("UniFormer: representation_size (the pre-logits layer of the classifier) is not built")
        if len(layers) != 4 or len(embed_dim) != 4 or min(layers) < 1:
            raise ValueError("UniFormer: four stages of at least one block each")
        if any(d % head_dim for d in embed_dim[2:]):
            raise ValueError(f"UniFormer: the widths of stages 3 and 4 {tuple(embed_dim[2:])} must be whole numbers of {head_dim}-wide heads")
        self.num_classes, self.use_checkpoint, self.checkpoint_num, self.windows = num_classes, use_checkpoint, checkpoint_num, windows
        self.num_features = self.embed_dim = embed_dim
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.patch_embed1 = PatchEmbed(img_size=img_size, patch_size=4, in_chans=in_chans, embed_dim=embed_dim[0])
        self.patch_embed2 = PatchEmbed(img_size=img_size // 4, patch_size=2, in_chans=embed_dim[0], embed_dim=embed_dim[1])
        self.patch_embed3 = PatchEmbed(img_size=img_size // 8, patch_size=2, in_chans=embed_dim[1], embed_dim=embed_dim[2])
        self.patch_embed4 = PatchEmbed(img_size=img_size // 16, patch_size=2, in_chans=embed_dim[2], embed_dim=embed_dim[3])
        num_heads = [dim // head_dim for dim in embed_dim]
        kw = dict(mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, norm_layer=norm_layer)
        for n, (cls, depth) in enumerate(zip((CBlock, CBlock, SABlock, SABlock), layers), 1):
            setattr(self, f"blocks{n}", nn.ModuleList([cls(dim=embed_dim[n - 1], num_heads=num_heads[n - 1], **kw) for _ in range(depth)]))
            setattr(self, f"norm{n}", norm_layer(embed_dim[n - 1]))
        self.pre_logits = nn.Identity()
        self.eval()
        if isinstance(pretrained_path, str):
            from anyedit_amd.checkpoints import load_uniformer
            load_uniformer(self, pretrained_path)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("UniFormer: training mode is not built (BatchNorm runs on its running statistics, drop-path is an identity)")
        return super().train(False)

    def _norm(self, n):
        m = getattr(self, f"norm{n}")
        if ops.cache_stale(m, "_pk", *m.parameters()):
            m._pk = (_f32(m.weight), _f32(m.bias), m.eps)
        return m._pk

    @torch.no_grad()
    def _run(self, x, want_maps, want_rows):
        if x.dim() != 4 or x.dtype != torch.float32:
            raise TypeError(f"UniFormer: expected fp32 [B, {self.patch_embed1.proj.in_channels}, H, W], got {x.dtype} {tuple(x.shape)}")
        B, Cin, H, W = x.shape
        if Cin != self.patch_embed1.proj.in_channels:
            raise ValueError(f"UniFormer: expected {self.patch_embed1.proj.in_channels} input channels, got {Cin}")
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"UniFormer: a {H} x {W} image is refused: with a side below {MIN_SIDE} pixels the stride-32 map would be empty")
        out = []
        for n in range(1, 5):
            pe = getattr(self, f"patch_embed{n}")
            h, H, W = pe.from_pixels(x) if n == 1 else pe.from_rows(h, B, H, W)
            for blk in getattr(self, f"blocks{n}"):
                h = blk.rows(h, B, H, W)
            g, b, eps = self._norm(n)
            if want_maps:
                r = ops.layernorm_rows_nchw(h, g, b, eps, B, H, W, want_rows=want_rows)
                out.append((r[0], r[1], H, W) if want_rows else (r, None, H, W))
            else:
                out.append((None, ops.layernorm(h, g, b, eps), H, W))
        return out

    def forward_features(self, x):
        return tuple(m for m, _, _, _ in self._run(x, True, False))

    def forward(self, x):
        return self.forward_features(x)

    def forward_rows(self, x):
        return [(r, h, w) for _, r, h, w in self._run(x, False, True)]

    def forward_both(self, x):
        """(the four fp32 maps, the four (rows, h, w)) from one pass: each output launch writes both forms."""
        res = self._run(x, True, True)
        return tuple(m for m, _, _, _ in res), [(r, h, w) for _, r, h, w in res]
