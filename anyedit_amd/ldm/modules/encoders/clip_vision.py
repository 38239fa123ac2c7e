"""train.py:404, 689-691 — the frozen CLIP vision tower on the HIP path: the image encoder that turns a reference image into the
[B, 1 + G, C] hidden states AnySD's adapter reads (`image_encoder(reference_clip_images, output_hidden_states=True).hidden_states[-2]`).

The tower is transformers' CLIPVisionModelWithProjection restated over the library:

    patch rows (im2col, rescale + normalise fused) -> patch GEMM (fp32 product) -> + class / position embeddings, pre_layrnorm   = hidden_states[0]
    L pre-LN layers, each
        h = LayerNorm1(x) -> q|k|v (ONE [3C, C] GEMM, +bias) -> attention over all 1 + G tokens -> out_proj (+bias, +x)          = x'
        h = LayerNorm2(x') -> fc1 (fp32 product) -> +bias, quick-GELU / GELU -> fc2 (+bias, +x')                                   = next x
    post_layernorm of the class row only -> visual_projection (no bias)                                                           = image_embeds

Kernels: `ops.clip_patch_rows`, `ops.clip_vision_embed_ln`, `ops.clip_vision_pool_ln` (csrc/clip_vision.hip holds these three), `ops.gemm`,
`ops.layernorm`, `ops.attention`, `ops.bias_act`.  Every activation stored between two launches is bf16; the points are marked `# bf16:`
below and tests/clip_vision_ref.py rounds at exactly those points for its control.

Parameters carry the checkpoint's own names (`vision_model.embeddings.*`, `vision_model.pre_layrnorm.*` — the checkpoint's spelling —,
`vision_model.encoder.layers.N.*`, `vision_model.post_layernorm.*`, `visual_projection.weight`), so `load_state_dict` of a Hugging Face
file fills the tower.  Nothing here ever reaches for a network: the geometry comes from `config` (a dict).

One call on a given (B, H, W) makes no allocation and no host synchronisation after the first, runs on the current stream only and may
be captured in a graph: its buffers (the returned tensors included) are static per shape.
"""
import types

import torch
import torch.nn as nn

from anyedit_amd import ops
from anyedit_amd.ldm.modules.encoders.modules import _ACTS, _Encoder

BF16 = torch.bfloat16

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_PROCESSOR = dict(num_channels=3, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD, rescale_factor=1.0 / 255.0)
# laion/CLIP-ViT-H-14-laion2B-s32B-b79K's vision tower: the IP-Adapter image encoder (models/image_encoder), what clip_dim = 1280 implies
CLIP_VIT_H_14_VISION = dict(hidden_size=1280, num_hidden_layers=32, num_attention_heads=16, intermediate_size=5120, patch_size=14, image_size=224,
                            hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1024, **_PROCESSOR)
# openai/clip-vit-large-patch14's vision tower
CLIP_VIT_L_14_VISION = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, patch_size=14, image_size=224,
                            hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=768, **_PROCESSOR)
_ATTN_HEAD_DIMS = (8, 16, 32, 40, 48, 64, 80, 96, 128, 160)   # ae_attn_fwd_bf16's instantiations
_LN_CMAX = 2048                                               # csrc/clip_vision.hip: a row lives in one wave's registers
_FAST_HEAD_DIMS = (40, 80, 160)                               # head dims ae_attn_fwd_bf16 hands to attention_fast.hip
_FAST_KEY_TILE = 64                                           # its LDS tile: keys per step


def attention_rows(qkv, B, H, N, D, out, ones=None):
    """The tower's attention launch: `ops.attention` over packed q | k | v rows [B*N, 3*H*D], all N tokens, no mask in effect.

    Below one 64-key tile at the head dims of attention_fast.hip (40 / 80 / 160) an all-ones key mask [B, N] (uint8; `ones`, made here when
    not given) is passed: a mask sends ae_attn_fwd_bf16 to the general kernel of attention.hip.  The fast kernel rounds Q * scale * log2(e) to
    bf16 in front of the logit MFMA; with few keys to share the probability mass that rounding leaves the float64 bound of the attention
    routes (N = 10, D = 80: 1.0014 of it), and below one tile the fast kernel has nothing to amortise anyway.  The
    general kernel scales the fp32 logits.  The full-size towers (257 tokens) are not affected."""
    C = H * D
    st = (N * 3 * C, D, 3 * C)
    mask = None
    if D in _FAST_HEAD_DIMS and N < _FAST_KEY_TILE:
        mask = ones if ones is not None else torch.ones(B, N, dtype=torch.uint8, device=qkv.device)
    return ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], B, H, N, N, D, D ** -0.5, st, st, st, out=out, key_mask=mask)


class CLIPVisionOutput:
    """What transformers' CLIPVisionModelWithProjection returns, as far as the reference reads it: attributes, and indexing in transformers'
    order (image_embeds, last_hidden_state, hidden_states)."""

    def __init__(self, image_embeds, last_hidden_state, hidden_states=None, pooler_output=None):
        self.image_embeds, self.last_hidden_state, self.hidden_states = image_embeds, last_hidden_state, hidden_states
        self.pooler_output = pooler_output     # post_layernorm of the class rows, what visual_projection reads (not part of the indexing)

    def __getitem__(self, i):
        return tuple(v for v in (self.image_embeds, self.last_hidden_state, self.hidden_states) if v is not None)[i]


class _VisionEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C, P = cfg["hidden_size"], cfg["patch_size"]
        self.class_embedding = nn.Parameter(torch.randn(C))
        self.patch_embedding = nn.Conv2d(cfg["num_channels"], C, kernel_size=P, stride=P, bias=False)
        self.position_embedding = nn.Embedding((cfg["image_size"] // P) ** 2 + 1, C)
        # checkpoints written by older transformers carry the arange buffer `position_ids`: accepted and ignored
        self._register_load_state_dict_pre_hook(self._drop_position_ids)

    @staticmethod
    def _drop_position_ids(state_dict, prefix, *_):
        state_dict.pop(prefix + "position_ids", None)


class _VisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.embeddings = _VisionEmbeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(C, eps=eps)
        self.encoder = _Encoder(cfg)           # the text tower's layer classes: same parameters, same packed images
        self.post_layernorm = nn.LayerNorm(C, eps=eps)


class CLIPVisionModelWithProjection(nn.Module):
    """transformers' class of that name (vision_model.{embeddings, pre_layrnorm, encoder.layers, post_layernorm}, visual_projection) on HIP.
    `config`: overrides of `CLIP_VIT_H_14_VISION`."""

    def __init__(self, config=None):
        super().__init__()
        cfg = dict(CLIP_VIT_H_14_VISION)
        cfg.update(config or {})
        C, H = cfg["hidden_size"], cfg["num_attention_heads"]
        if C % H or C // H not in _ATTN_HEAD_DIMS:
            raise ValueError(f"CLIPVisionModelWithProjection: head_dim {C}/{H} is not one ae_attn_fwd_bf16 supports {_ATTN_HEAD_DIMS}")
        if cfg["hidden_act"] not in _ACTS:
            raise ValueError(f"CLIPVisionModelWithProjection: hidden_act {cfg['hidden_act']!r} (supported: {sorted(_ACTS)})")
        if cfg["patch_size"] <= 0 or cfg["image_size"] % cfg["patch_size"]:
            raise ValueError(f"CLIPVisionModelWithProjection: image_size {cfg['image_size']} is not a multiple of patch_size {cfg['patch_size']}")
        if C % 8 or C > _LN_CMAX:
            raise ValueError(f"CLIPVisionModelWithProjection: hidden_size {C} must be a multiple of 8 and at most {_LN_CMAX} (the embedding / pooling LayerNorm kernels)")
        if len(cfg["image_mean"]) != cfg["num_channels"] or len(cfg["image_std"]) != cfg["num_channels"]:
            raise ValueError("CLIPVisionModelWithProjection: image_mean / image_std need one value per channel")
        self.config = cfg
        self.vision_model = _VisionTransformer(cfg)
        self.visual_projection = nn.Linear(C, cfg["projection_dim"], bias=False)
        self._ws = {}

    @property
    def device(self):
        return self.visual_projection.weight.device

    @property
    def hidden_size(self):
        return self.config["hidden_size"]

    # ---- caches ---------------------------------------------------------------------------------------------------------------
    def _tables(self):
        v = self.vision_model
        e = v.embeddings
        src = (e.class_embedding, e.patch_embedding.weight, e.position_embedding.weight, v.pre_layrnorm.weight, v.pre_layrnorm.bias,
               v.post_layernorm.weight, v.post_layernorm.bias, self.visual_projection.weight)
        if ops.cache_stale(self, "_pk", *src):
            f = lambda t: t.detach().float().contiguous()
            dev = e.class_embedding.device
            self._pk = types.SimpleNamespace(
                wpatch=ops.pack_patch_embedding(e.patch_embedding.weight),            # [C, Kpad] bf16, zero-padded, packed once
                cls=f(e.class_embedding), pos=f(e.position_embedding.weight),         # fp32: added to the fp32 patch product
                g0=f(v.pre_layrnorm.weight), e0=f(v.pre_layrnorm.bias), g1=f(v.post_layernorm.weight), e1=f(v.post_layernorm.bias),
                wproj=ops.pack_linear(self.visual_projection.weight),
                mean=torch.tensor(self.config["image_mean"], dtype=torch.float32, device=dev),
                std=torch.tensor(self.config["image_std"], dtype=torch.float32, device=dev))
        return self._pk

    def weights_token(self):
        """Changes whenever any parameter of the tower does (callers cache encodings against it)."""
        return ops.weights_token(*self.parameters())

    def _workspace(self, B, S, dev):
        key = (B, S, S, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            cfg = self.config
            P, C, I, L = cfg["patch_size"], cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
            G = (S // P) ** 2
            M = B * (G + 1)
            e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
            ws = self._ws[key] = types.SimpleNamespace(
                rows=e(B * G, ops.clip_patch_kpad(cfg["num_channels"], P)), patch=e(B * G, C, dt=torch.float32), hs=[e(M, C) for _ in range(L + 1)],
                h=e(M, C), qkv=e(M, 3 * C), att=e(M, C), mid=e(M, C), u=e(M, I, dt=torch.float32), act=e(M, I), pooled=e(B, C),
                embeds=e(B, cfg["projection_dim"]), ones=torch.ones(B, G + 1, dtype=torch.uint8, device=dev))
        return ws

    # ---- the tower ------------------------------------------------------------------------------------------------------------
    def _check_pixels(self, px):
        cfg = self.config
        S = cfg["image_size"]
        if not isinstance(px, torch.Tensor) or px.dim() != 4:
            raise ValueError(f"pixel_values: expected a [B, {cfg['num_channels']}, {S}, {S}] tensor")
        if px.dtype not in (torch.float32, BF16, torch.uint8):
            raise TypeError(f"pixel_values: expected fp32 / bf16 (already normalised) or uint8 (raw) pixels, got {px.dtype}")
        if px.shape[0] < 1 or px.shape[1] != cfg["num_channels"] or px.shape[2] != S or px.shape[3] != S:
            raise ValueError(f"pixel_values: expected [B, {cfg['num_channels']}, {S}, {S}], got {tuple(px.shape)} (resizing and position-embedding "
                             f"interpolation are out of scope: bring the image to the model resolution first)")
        if not px.is_cuda or self.device.type != "cuda":
            raise ValueError("CLIPVisionModelWithProjection: the tower runs on the GPU only (anyedit_amd has no CPU path); move the tower and "
                             "pixel_values with .to('cuda')")
        if not px.is_contiguous():
            raise ValueError("pixel_values: expected a contiguous tensor (a copy would be an allocation inside the encode)")

    @torch.no_grad()
    def run(self, pixel_values, n_layers=None):
        """Embeds `pixel_values` and runs the first `n_layers` layers (all by default); returns the workspace with `ws.hs[0 .. n_layers]` filled:
        hs[0] the token rows after pre_layrnorm, hs[i] the residual stream after layer i (transformers' `hidden_states`)."""
        cfg = self.config
        self._check_pixels(pixel_values)
        B, S = pixel_values.shape[0], pixel_values.shape[2]
        C, H, P = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"]
        D, eps, act = C // H, cfg["layer_norm_eps"], _ACTS[cfg["hidden_act"]]
        L = cfg["num_hidden_layers"] if n_layers is None else n_layers
        N = (S // P) ** 2 + 1
        t = self._tables()
        ws = self._workspace(B, S, self.device)
        hs = ws.hs
        if pixel_values.dtype == torch.uint8:     # raw pixels: the image processor's rescale + normalise, fused into the im2col
            ops.clip_patch_rows(pixel_values, P, cfg["rescale_factor"], t.mean, t.std, out=ws.rows)          # bf16: normalised pixels as patch rows
        else:
            ops.clip_patch_rows(pixel_values, P, out=ws.rows)                                        # bf16: normalised pixels as patch rows
        ops.gemm(ws.rows, t.wpatch, None, out_f32=True, out=ws.patch)                                # fp32: patch embedding product (class / position add and pre_layrnorm follow in fp32)
        ops.clip_vision_embed_ln(ws.patch, t.cls, t.pos, t.g0, t.e0, eps, B, out=hs[0])             # bf16: token rows after pre_layrnorm (hidden_states[0])
        qkv = ws.qkv
        for i in range(L):
            p = self.vision_model.encoder.layers[i].packed()
            ops.layernorm(hs[i], p.g1, p.e1, eps, out=ws.h)                                        # bf16: LayerNorm1 output
            ops.gemm(ws.h, p.wqkv, p.bqkv, out=qkv)                                                # bf16: packed q | k | v
            attention_rows(qkv, B, H, N, D, ws.att, ws.ones)                                       # bf16: attention output
            ops.gemm(ws.att, p.wo, p.bo, residual=hs[i], out=ws.mid)                               # bf16: residual stream after the attention add
            ops.layernorm(ws.mid, p.g2, p.e2, eps, out=ws.h)                                       # bf16: LayerNorm2 output
            ops.gemm(ws.h, p.w1, None, out_f32=True, out=ws.u)                                     # fp32: fc1 product (bias and activation follow in fp32)
            ops.bias_act(ws.u, p.b1, act, out=ws.act)                                              # bf16: activated hidden values
            ops.gemm(ws.act, p.w2, p.b2, residual=ws.mid, out=hs[i + 1])                           # bf16: residual stream after the MLP add
        return ws

    def forward(self, pixel_values, output_hidden_states=False):
        """transformers' call: returns a `CLIPVisionOutput` with image_embeds [B, projection_dim], last_hidden_state [B, N, C] (the last layer's
        output with NO final norm, as transformers returns it: post_layernorm touches the pooled row only) and, on request, hidden_states
        (L + 1 tensors, index 0 after pre_layrnorm).  All are bf16 views of the static workspace of this (B, H, W): valid until the next
        call of that shape — `.clone()` what you keep."""
        ws = self.run(pixel_values)
        cfg = self.config
        B, L = pixel_values.shape[0], cfg["num_hidden_layers"]
        N = ws.hs[0].shape[0] // B
        t = self._tables()
        ops.clip_vision_pool_ln(ws.hs[L], N, t.g1, t.e1, cfg["layer_norm_eps"], out=ws.pooled)      # bf16: post_layernorm of the class rows
        ops.gemm(ws.pooled, t.wproj, None, out=ws.embeds)                                          # bf16: image_embeds
        return CLIPVisionOutput(ws.embeds, ws.hs[L].view(B, N, -1), tuple(h.view(B, N, -1) for h in ws.hs) if output_hidden_states else None, ws.pooled)

    def encode_pixels(self, pixel_values, layer=-2):
        """`self(pixel_values, output_hidden_states=True).hidden_states[layer]` -> [B, N, C] bf16, running only the layers it needs (-2: L - 1
        layers, no pooling, no projection; train.py:689-691).

        pixel_values: [B, 3, S, S] on the GPU, contiguous; fp32 / bf16 already normalised, or uint8 raw pixels (rescaled and normalised with
        the config's rescale_factor / image_mean / image_std inside the im2col kernel).
        The result is a view of this shape's static buffer (no allocation and no host synchronisation after the first call, capturable in a
        graph): it is overwritten by the next call with the same (B, H, W) — `.clone()` it to keep it; `MoE.reference_embeds` does."""
        L = self.config["num_hidden_layers"]
        idx = layer if layer >= 0 else L + 1 + layer
        if not 0 <= idx <= L:
            raise ValueError(f"encode_pixels: layer {layer} is outside hidden_states[0 .. {L}]")
        ws = self.run(pixel_values, n_layers=idx)
        B = pixel_values.shape[0]
        return ws.hs[idx].view(B, ws.hs[idx].shape[0] // B, -1)
