"""ldm/modules/encoders/modules.py:279-315 — FrozenDinoV2Encoder on the HIP path: the image encoder that turns a 224x224 reference crop into
the [B, 257, 1024] context AnyDoor's ControlNet and UNet cross-attend to (`model.get_learned_conditioning(clip_input)`,
visual_reference_tool.py:199-205).

The tower is `DinoVisionTransformer` (AnyEdit_Collection/other_modules/depth_anything_v2/dinov2.py:44-328; the class Depth-Anything runs
under its DPT head in the ViT-S/B/L geometries) restated over the library:

    patch rows (im2col, ImageNet normalise fused on request) -> patch GEMM (fp32 product) -> + bias, class token, interpolated position table = x_0
    depth blocks, each
        h = norm1(x) -> q|k|v (ONE [3C, C] GEMM, +bias) -> attention over all 1 + G tokens -> ls1 * proj (+bias), +x                    = x'
        h = norm2(x') -> w12 (fp32 product) -> +bias, silu(x1) * x2 -> ls2 * w3 (+bias), +x'          (swiglufused)
                      -> fc1 (fp32 product) -> +bias, GELU          -> ls2 * fc2 (+bias), +x'          (mlp)                              = next x
    norm of every row                                                                                                                = x_norm

LayerScale costs no launch: `gamma[:, None] * W` and `gamma * b` are folded into `attn.proj` and `mlp.w3` / `mlp.fc2` in fp32 when the
weights are packed, before the bf16 rounding (which is relative, so the accuracy is that of the unfolded product); the fold is rebuilt when a
parameter changes.  Kernels: `ops.clip_patch_rows`, `ops.dino_embed`, `ops.swiglu` (csrc/dino_vision.hip holds the last two), `ops.gemm`,
`ops.layernorm`, `ops.attention` (through `clip_vision.attention_rows`), `ops.bias_act`.  Every activation stored between two launches is
bf16; the points are marked `# bf16:` below and tests/dino_ref.py rounds at exactly those points for its control.

Parameters carry the checkpoint's own names with block_chunks = 0 (`cls_token`, `pos_embed`, `mask_token`, `patch_embed.proj.*`,
`blocks.N.{norm1, attn.qkv, attn.proj, ls1.gamma, norm2, mlp.{w12, w3} | mlp.{fc1, fc2}, ls2.gamma}`, `norm.*`), so `load_state_dict` of a
`dinov2_vit*14_pretrain.pth` fills the tower.  Nothing here ever reaches for a network or opens a file: the geometry comes from `config`.

One call on a given (B, H, W) makes no allocation and no host synchronisation after the first with the same arguments, runs on the current
stream only and may be captured in a graph: its buffers (the returned tensors included) are static per shape.
"""
import math
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from anyedit_amd import ops
from anyedit_amd.ldm.modules.encoders.clip_vision import _ATTN_HEAD_DIMS, _LN_CMAX, attention_rows
from anyedit_amd.ldm.modules.encoders.modules import AbstractEncoder

BF16 = torch.bfloat16

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # modules.py:292-293
IMAGENET_STD = (0.229, 0.224, 0.225)
_COMMON = dict(patch_size=14, img_size=518, in_chans=3, mlp_ratio=4.0, init_values=1.0, interpolate_offset=0.1, interpolate_antialias=False,
               num_register_tokens=0, layer_norm_eps=1e-6)
# dinov2.py:398-415 DINOv2(model_name): vitg is what hubconf.dinov2_vitg14 builds (modules.py:285)
DINOV2_VITG14 = dict(embed_dim=1536, depth=40, num_heads=24, ffn_layer="swiglufused", **_COMMON)
DINOV2_VITL14 = dict(embed_dim=1024, depth=24, num_heads=16, ffn_layer="mlp", **_COMMON)
DINOV2_VITB14 = dict(embed_dim=768, depth=12, num_heads=12, ffn_layer="mlp", **_COMMON)
DINOV2_VITS14 = dict(embed_dim=384, depth=12, num_heads=6, ffn_layer="mlp", **_COMMON)
_SWIGLU = ("swiglufused", "swiglu")


def swiglu_hidden(C, mlp_ratio=4.0):
    """dinov2_layers/swiglu_ffn.py:57: the hidden width of SwiGLUFFNFused (ViT-g: 4096)."""
    return (int(int(C * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def interpolated_pos_embed(pos_embed, gh, gw, offset=0.1):
    """dinov2.py:179-210 interpolate_pos_encoding for a grid of gh x gw patches: pos_embed [1, 1 + N, C] (or [1 + N, C]) -> fp32 [1 + gh gw, C].
    The class row is untouched; the N = n x n patch rows are resampled with torch's bicubic interpolation, scale_factor = ((gh + offset) / n,
    (gw + offset) / n), no antialias.  The native square grid is returned as it is.  A pure function of its arguments; runs wherever
    `pos_embed` lives (CPU included)."""
    pe = pos_embed.detach().float()
    pe = pe[0] if pe.dim() == 3 else pe
    N, C = pe.shape[0] - 1, pe.shape[1]
    n = int(math.sqrt(N))
    if n * n != N:
        raise ValueError(f"interpolated_pos_embed: {N} patch positions are not a square grid")
    if gh <= 0 or gw <= 0:
        raise ValueError(f"interpolated_pos_embed: bad grid {gh}x{gw}")
    if gh * gw == N and gh == gw:
        return pe.contiguous()
    sqrt_n = math.sqrt(N)
    sy, sx = float(gh + offset) / sqrt_n, float(gw + offset) / sqrt_n
    grid = F.interpolate(pe[1:].reshape(1, n, n, C).permute(0, 3, 1, 2), scale_factor=(sy, sx), mode="bicubic", antialias=False)
    if tuple(grid.shape[-2:]) != (gh, gw):
        raise ValueError(f"interpolated_pos_embed: the interpolation gave {tuple(grid.shape[-2:])} for a {gh}x{gw} grid (offset {offset})")
    return torch.cat([pe[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, C)], 0).contiguous()


class _PatchEmbed(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        P = cfg["patch_size"]
        self.proj = nn.Conv2d(cfg["in_chans"], cfg["embed_dim"], kernel_size=P, stride=P)


class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.qkv, self.proj = nn.Linear(C, 3 * C), nn.Linear(C, C)


class _LayerScale(nn.Module):
    def __init__(self, C, init_values):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(C))


class _Mlp(nn.Module):
    def __init__(self, C, hidden):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, hidden), nn.Linear(hidden, C)


class _SwiGLUFFN(nn.Module):
    def __init__(self, C, hidden):
        super().__init__()
        self.w12, self.w3 = nn.Linear(C, 2 * hidden), nn.Linear(hidden, C)


class _Block(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C, eps = cfg["embed_dim"], cfg["layer_norm_eps"]
        self.norm1 = nn.LayerNorm(C, eps=eps)
        self.attn = _Attention(C)
        self.norm2 = nn.LayerNorm(C, eps=eps)
        self.swiglu = cfg["ffn_layer"] in _SWIGLU
        self.mlp = _SwiGLUFFN(C, swiglu_hidden(C, cfg["mlp_ratio"])) if self.swiglu else _Mlp(C, int(C * cfg["mlp_ratio"]))
        if cfg["init_values"]:                 # block.py:65, 77: None or 0 => no LayerScale (and no gamma in the checkpoint)
            self.ls1, self.ls2 = _LayerScale(C, cfg["init_values"]), _LayerScale(C, cfg["init_values"])

    def packed(self):
        """bf16 weight images + fp32 biases / affine vectors of this block, LayerScale folded into the two output projections in fp32;
        rebuilt when any of its tensors changes."""
        if ops.cache_stale(self, "_pk", *self.parameters()):
            f = lambda t: t.detach().float().contiguous()
            a, m = self.attn, self.mlp
            g1 = f(self.ls1.gamma) if hasattr(self, "ls1") else None
            g2 = f(self.ls2.gamma) if hasattr(self, "ls2") else None

            def fold(lin, g):                  # ls(W x + b) = (gamma[:, None] * W) x + gamma * b
                w, b = f(lin.weight), f(lin.bias)
                return (ops.pack_linear(w), b) if g is None else (ops.pack_linear(g[:, None] * w), (g * b).contiguous())

            first, last = (m.w12, m.w3) if self.swiglu else (m.fc1, m.fc2)
            wo, bo = fold(a.proj, g1)
            w2, b2 = fold(last, g2)
            self._pk = types.SimpleNamespace(wqkv=ops.pack_linear(a.qkv.weight), bqkv=f(a.qkv.bias), wo=wo, bo=bo, w1=ops.pack_linear(first.weight),
                                             b1=f(first.bias), w2=w2, b2=b2, g1=f(self.norm1.weight), e1=f(self.norm1.bias),
                                             g2=f(self.norm2.weight), e2=f(self.norm2.bias))
        return self._pk


class DinoVisionTransformer(nn.Module):
    """dinov2.py:44-328 on HIP.  `config`: overrides of `DINOV2_VITG14` (the reference constructor's argument names)."""

    def __init__(self, config=None):
        super().__init__()
        cfg = dict(DINOV2_VITG14)
        cfg.update(config or {})
        C, H, P = cfg["embed_dim"], cfg["num_heads"], cfg["patch_size"]
        if cfg["num_register_tokens"]:
            raise ValueError(f"DinoVisionTransformer: num_register_tokens={cfg['num_register_tokens']}: register tokens are not built (the reference's towers have none)")
        if cfg["interpolate_antialias"]:
            raise ValueError("DinoVisionTransformer: interpolate_antialias=True is not built (the reference interpolates the position table without it)")
        if cfg["ffn_layer"] == "identity":
            raise ValueError("DinoVisionTransformer: ffn_layer='identity' is not built (supported: 'mlp', 'swiglufused', 'swiglu')")
        if cfg["ffn_layer"] not in _SWIGLU + ("mlp",):
            raise ValueError(f"DinoVisionTransformer: ffn_layer {cfg['ffn_layer']!r} (supported: 'mlp', 'swiglufused', 'swiglu')")
        if C % 8 or C > _LN_CMAX:
            raise ValueError(f"DinoVisionTransformer: embed_dim {C} must be a multiple of 8 and at most {_LN_CMAX}")
        if C % H or C // H not in _ATTN_HEAD_DIMS:
            raise ValueError(f"DinoVisionTransformer: head_dim {C}/{H} is not one ae_attn_fwd_bf16 supports {_ATTN_HEAD_DIMS}")
        if P <= 0 or cfg["img_size"] % P:
            raise ValueError(f"DinoVisionTransformer: img_size {cfg['img_size']} is not a multiple of patch_size {P}")
        if int(C * cfg["mlp_ratio"]) % 8:
            raise ValueError(f"DinoVisionTransformer: hidden width {int(C * cfg['mlp_ratio'])} must be a multiple of 8")
        self.config = cfg
        self.embed_dim = self.num_features = C
        self.patch_size, self.num_heads, self.n_blocks = P, H, cfg["depth"]
        self.num_register_tokens = 0
        self.patch_embed = _PatchEmbed(cfg)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, C))
        self.pos_embed = nn.Parameter(torch.zeros(1, (cfg["img_size"] // P) ** 2 + 1, C))
        self.blocks = nn.ModuleList([_Block(cfg) for _ in range(cfg["depth"])])
        self.norm = nn.LayerNorm(C, eps=cfg["layer_norm_eps"])
        self.mask_token = nn.Parameter(torch.zeros(1, C))      # in the checkpoint; only masked training reads it
        self._ws, self._pos = {}, {}

    @property
    def device(self):
        return self.cls_token.device

    # ---- caches ---------------------------------------------------------------------------------------------------------------
    def _tables(self):
        pe = self.patch_embed.proj
        if ops.cache_stale(self, "_pk", pe.weight, pe.bias, self.cls_token, self.norm.weight, self.norm.bias):
            f = lambda t: t.detach().float().contiguous()
            dev = self.cls_token.device
            self._pk = types.SimpleNamespace(
                wpatch=ops.pack_patch_embedding(pe.weight), bpatch=f(pe.bias), cls=f(self.cls_token).view(-1),   # bias / class token fp32: added to the fp32 patch product
                g=f(self.norm.weight), e=f(self.norm.bias),
                mean=torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=dev), std=torch.tensor(IMAGENET_STD, dtype=torch.float32, device=dev))
        return self._pk

    def pos_table(self, gh, gw):
        """The fp32 position table [1 + gh gw, C] of this grid: `interpolated_pos_embed`, once per grid and per value of `pos_embed`
        (computed on the host with the reference's own torch call, then moved to the tower's device)."""
        tok = ops.weights_token(self.pos_embed)
        hit = self._pos.get((gh, gw))
        if hit is None or hit[0] != tok:
            table = interpolated_pos_embed(self.pos_embed.detach().cpu(), gh, gw, self.config["interpolate_offset"])
            hit = self._pos[(gh, gw)] = (tok, table.to(self.pos_embed.device))
        return hit[1]

    def weights_token(self):
        """Changes whenever any parameter of the tower does (callers cache encodings against it)."""
        return ops.weights_token(*self.parameters())

    def _workspace(self, B, H, W, dev):
        key = (B, H, W, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            cfg = self.config
            P, C, L = cfg["patch_size"], cfg["embed_dim"], cfg["depth"]
            G = (H // P) * (W // P)
            M = B * (G + 1)
            swi = cfg["ffn_layer"] in _SWIGLU
            Hd = swiglu_hidden(C, cfg["mlp_ratio"]) if swi else int(C * cfg["mlp_ratio"])
            e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
            ws = self._ws[key] = types.SimpleNamespace(
                rows=e(B * G, ops.clip_patch_kpad(cfg["in_chans"], P)), patch=e(B * G, C, dt=torch.float32), hs=[e(M, C) for _ in range(L + 1)],
                h=e(M, C), qkv=e(M, 3 * C), att=e(M, C), mid=e(M, C), u=e(M, 2 * Hd if swi else Hd, dt=torch.float32), act=e(M, Hd),
                ones=torch.ones(B, G + 1, dtype=torch.uint8, device=dev), z={}, grid={}, px=None)
        return ws

    # ---- the tower ------------------------------------------------------------------------------------------------------------
    def _pixels(self, x):
        """Checks a tensor or a list of tensors (concatenated on dim 0 into the workspace's static buffer); returns (pixels, workspace)."""
        cfg = self.config
        P, Cin = cfg["patch_size"], cfg["in_chans"]
        parts = list(x) if isinstance(x, (list, tuple)) else [x]
        if not parts:
            raise ValueError("pixels: an empty list")
        for t in parts:
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"pixels: expected a [B, {Cin}, H, W] tensor or a list of them")
            if t.dtype != torch.float32:
                raise TypeError(f"pixels: expected fp32 pixels, got {t.dtype}")
            if t.shape[0] < 1 or t.shape[1] != Cin or tuple(t.shape[1:]) != tuple(parts[0].shape[1:]):
                raise ValueError(f"pixels: expected [B, {Cin}, H, W] tensors of one size, got {[tuple(p.shape) for p in parts]}")
        H, W = parts[0].shape[2:]
        if H < P or W < P or H % P or W % P:
            raise ValueError(f"pixels: image {H}x{W} is not a whole number of {P}x{P} patches (resizing and cropping stay with the caller)")
        if self.device.type != "cuda" or (len(parts) == 1 and not parts[0].is_cuda):
            raise ValueError("DinoVisionTransformer: the tower runs on the GPU only (anyedit_amd has no CPU path); move the tower and the pixels with .to('cuda')")
        if len(parts) == 1 and not parts[0].is_contiguous():
            raise ValueError("pixels: expected a contiguous tensor (a copy would be an allocation inside the encode)")
        B = sum(t.shape[0] for t in parts)
        ws = self._workspace(B, H, W, self.device)
        if len(parts) == 1:
            return parts[0], ws
        if ws.px is None:
            ws.px = torch.empty(B, Cin, H, W, dtype=torch.float32, device=self.device)
        o = 0
        for t in parts:                        # torch.cat(image, 0) of modules.py:302-303, into a static buffer
            ws.px[o:o + t.shape[0]].copy_(t)
            o += t.shape[0]
        return ws.px, ws

    @torch.no_grad()
    def run(self, x, n_blocks=None, normalize=False, masks=None):
        """Embeds the pixels and runs the first `n_blocks` blocks (all by default); returns the workspace with `ws.hs[0 .. n_blocks]` filled:
        hs[0] the token rows, hs[i] the residual stream after block i - 1.  normalize: (x - ImageNet mean) / std inside the patch launch."""
        if masks is not None:
            raise ValueError("DinoVisionTransformer: masks (masked patch tokens) are not built; mask_token is carried for the checkpoint only")
        cfg = self.config
        px, ws = self._pixels(x)
        B, H, W = px.shape[0], px.shape[2], px.shape[3]
        C, NH, P = cfg["embed_dim"], cfg["num_heads"], cfg["patch_size"]
        D, eps = C // NH, cfg["layer_norm_eps"]
        L = cfg["depth"] if n_blocks is None else n_blocks
        gh, gw = H // P, W // P
        N = gh * gw + 1
        t = self._tables()
        pos = self.pos_table(gh, gw)
        hs = ws.hs
        if normalize:
            ops.clip_patch_rows(px, P, 1.0, t.mean, t.std, out=ws.rows)                             # bf16: normalised pixels as patch rows
        else:
            ops.clip_patch_rows(px, P, out=ws.rows)                                                  # bf16: pixels as patch rows
        ops.gemm(ws.rows, t.wpatch, None, out_f32=True, out=ws.patch)                                # fp32: patch embedding product (bias, class token and position table follow in fp32)
        ops.dino_embed(ws.patch, t.bpatch, t.cls, pos, B, out=hs[0])                                 # bf16: token rows (no pre-norm)
        for i in range(L):
            blk = self.blocks[i]
            p = blk.packed()
            ops.layernorm(hs[i], p.g1, p.e1, eps, out=ws.h)                                        # bf16: norm1 output
            ops.gemm(ws.h, p.wqkv, p.bqkv, out=ws.qkv)                                             # bf16: packed q | k | v
            attention_rows(ws.qkv, B, NH, N, D, ws.att, ws.ones)                                   # bf16: attention output
            ops.gemm(ws.att, p.wo, p.bo, residual=hs[i], out=ws.mid)                               # bf16: residual stream after the attention add (ls1 folded)
            ops.layernorm(ws.mid, p.g2, p.e2, eps, out=ws.h)                                       # bf16: norm2 output
            ops.gemm(ws.h, p.w1, None, out_f32=True, out=ws.u)                                     # fp32: w12 / fc1 product (bias and activation follow in fp32)
            if blk.swiglu:
                ops.swiglu(ws.u, p.b1, out=ws.act)                                                 # bf16: gated hidden values
            else:
                ops.bias_act(ws.u, p.b1, ops.ACT_GELU, out=ws.act)                                 # bf16: activated hidden values
            ops.gemm(ws.act, p.w2, p.b2, residual=ws.mid, out=hs[i + 1])                           # bf16: residual stream after the FFN add (ls2 folded)
        return ws

    def _normed(self, ws, index):
        """norm(hs[index]) -> this workspace's static buffer for that index."""
        z = ws.z.get(index)
        if z is None:
            z = ws.z[index] = torch.empty_like(ws.hs[index])
        t = self._tables()
        return ops.layernorm(ws.hs[index], t.g, t.e, self.config["layer_norm_eps"], out=z)          # bf16: final norm output

    def forward_features(self, x, masks=None, normalize=False):
        """dinov2.py:253-269: dict of x_norm_clstoken [B, C], x_norm_regtokens [B, 0, C], x_norm_patchtokens [B, G, C], x_prenorm [B, 1 + G, C]
        and masks (None).  All bf16 views of the static workspace of this (B, H, W): valid until the next call of that shape."""
        ws = self.run(x, normalize=normalize, masks=masks)
        L, C = self.config["depth"], self.embed_dim
        B = ws.ones.shape[0]
        z = self._normed(ws, L).view(B, -1, C)
        return {"x_norm_clstoken": z[:, 0], "x_norm_regtokens": z[:, 1:1], "x_norm_patchtokens": z[:, 1:], "x_prenorm": ws.hs[L].view(B, -1, C),
                "masks": None}

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        """dinov2.py:297-321: the outputs of the last `n` blocks (int) or of the blocks listed in `n`, patch tokens only, optionally normed,
        reshaped to [B, C, gh, gw] and paired with their class tokens.  Runs only as many blocks as the deepest requested one needs."""
        L = self.config["depth"]
        take = list(range(L - n, L)) if isinstance(n, int) else sorted(set(int(i) for i in n))
        if not take or take[0] < 0 or take[-1] >= L:
            raise ValueError(f"get_intermediate_layers: blocks {n} are outside [0, {L})")
        ws = self.run(x, n_blocks=take[-1] + 1)
        B, C, P = ws.ones.shape[0], self.embed_dim, self.patch_size
        outs = [(self._normed(ws, i + 1) if norm else ws.hs[i + 1]).view(B, -1, C) for i in take]
        cls = [o[:, 0] for o in outs]
        patches = [o[:, 1:] for o in outs]
        if reshape:
            px = x[0] if isinstance(x, (list, tuple)) else x
            gh, gw = px.shape[2] // P, px.shape[3] // P
            moved = []
            for i, o in zip(take, patches):
                g = ws.grid.get((i, norm))
                if g is None:
                    g = ws.grid[(i, norm)] = torch.empty(B, C, gh, gw, dtype=BF16, device=o.device)
                moved.append(g.copy_(o.reshape(B, gh, gw, C).permute(0, 3, 1, 2)))
            patches = moved
        return tuple(zip(patches, cls)) if return_class_token else tuple(patches)

    def forward(self, x, masks=None):
        """dinov2.py:323-328 (is_training False): the normed class token [B, C]."""
        return self.forward_features(x, masks)["x_norm_clstoken"]


class FrozenDinoV2Encoder(AbstractEncoder):
    """Uses the DINOv2 encoder for image (modules.py:279-315), on the HIP path: `model` the tower, `projector` = Linear(embed_dim, 1024).
    `config`: overrides of `DINOV2_VITG14`.  Weights come from `load_state_dict` / `checkpoints.load_dinov2`; no file is opened here."""

    def __init__(self, config=None, projector_out=1024, device="cuda", freeze=True):
        super().__init__()
        if projector_out <= 0 or projector_out % 4:
            raise ValueError(f"FrozenDinoV2Encoder: projector_out {projector_out} must be a positive multiple of 4")
        self.model = DinoVisionTransformer(config)
        self.projector = nn.Linear(self.model.embed_dim, projector_out)
        self._uncond = {}
        if freeze:
            self.freeze()

    def freeze(self):
        self.model.eval()
        for param in self.model.parameters():
            param.requires_grad = False

    def weights_token(self):
        return ops.weights_token(*self.parameters())

    def _projector(self):
        p = self.projector
        if ops.cache_stale(self, "_pk", p.weight, p.bias):
            self._pk = types.SimpleNamespace(w=ops.pack_linear(p.weight), b=p.bias.detach().float().contiguous())
        return self._pk

    @torch.no_grad()
    def encode_pixels(self, image):
        """image: [B, 3, H, W] fp32 in [0, 1] on the GPU (or a list of such tensors, concatenated on dim 0); H and W multiples of the patch.
        Returns projector(cat([x_norm_clstoken[:, None], x_norm_patchtokens], 1)) as [B, 1 + G, projector_out] bf16, the ImageNet
        normalisation done inside the patch launch.  The result is a view of this shape's static buffer (no allocation and no host
        synchronisation after the first call, capturable in a graph): the next call with the same (B, H, W) overwrites it."""
        tw = self.model
        ws = tw.run(image, normalize=True)
        L = tw.config["depth"]
        z = tw._normed(ws, L)                                                                        # class row first, then the patch rows: the cat of modules.py:310 is the buffer itself
        p = self._projector()
        if getattr(ws, "hint", None) is None or ws.hint.shape[1] != p.w.shape[0]:
            ws.hint = torch.empty(z.shape[0], p.w.shape[0], dtype=BF16, device=z.device)
        ops.gemm(z, p.w, p.b, out=ws.hint)                                                          # bf16: projected hint
        B = ws.ones.shape[0]
        return ws.hint.view(B, -1, p.w.shape[0])

    def forward(self, image):
        """modules.py:301-312.  A copy the caller owns (the conditional and the unconditional hint of one edit have the same shape)."""
        return self.encode_pixels(image).clone()

    def encode(self, image):
        return self(image)

    @torch.no_grad()
    def unconditional(self, n, size=(224, 224)):
        """The encoding of `n` all-zero images (visual_reference_tool.py:205 `get_learned_conditioning([torch.zeros((1, 3, 224, 224))] * n)`):
        computed once per (n, size), served from a cache until a weight of the encoder changes."""
        H, W = (size, size) if isinstance(size, int) else size
        tok = self.weights_token()
        hit = self._uncond.get((n, H, W))
        if hit is None or hit[0] != tok:
            zeros = torch.zeros(n, self.model.config["in_chans"], H, W, dtype=torch.float32, device=self.model.device)
            hit = self._uncond[(n, H, W)] = (tok, self.encode_pixels(zeros).clone())
        return hit[1]
