"""ldm/modules/encoders/modules.py:107-150 — FrozenCLIPEmbedder on the HIP path: the CLIP text tower that turns an instruction into the
[B, 77, C] hidden states the UNet's cross-attention reads.

The tower is transformers' CLIPTextModel restated over the library: 12 pre-LN layers, each

    h = LayerNorm1(x) -> q|k|v (ONE [3C, C] GEMM, +bias) -> causal attention -> out_proj (+bias, +x)          = x'
    h = LayerNorm2(x') -> fc1 (fp32 product) -> +bias, quick-GELU / GELU -> fc2 (+bias, +x')                   = next x

then the final LayerNorm.  Kernels: `ops.clip_embed`, `ops.layernorm`, `ops.gemm`, `ops.attention_causal_short`, `ops.bias_act`,
`ops.clip_pool_eos` (csrc/clip_text.hip holds the new ones).  Every activation stored between two launches is bf16; the points are
marked `# bf16:` below and tests/clip_ref.py rounds at exactly those points for its control.

Parameters carry the names SD-1.5 checkpoints use under `cond_stage_model.` (`transformer.text_model.*`), so the `load_state_dict` that
fills the UNet and the VAE fills the tower too.  Nothing here ever reaches for a network: the geometry comes from `config` (a dict), the
tokenizer is an object the caller passes in (or a LOCAL directory given as `version`).

One `encode_ids` call on a given [B, N] makes no allocation and no host synchronisation after the first, runs on the current stream only,
and may be captured in a graph: its buffers (the returned tensor included) are static per shape.
"""
import os
import types

import torch
import torch.nn as nn

from anyedit_amd import ops

BF16 = torch.bfloat16

# the text geometry of openai/clip-vit-large-patch14 (what SD-1.5 / AnyEdit checkpoints carry under cond_stage_model)
CLIP_VIT_L_TEXT = dict(vocab_size=49408, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                       max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407, bos_token_id=49406,
                       pad_token_id=49407)
_ACTS = {"quick_gelu": ops.ACT_QUICK_GELU, "gelu": ops.ACT_GELU}


class CLIPTextOutput:
    """What transformers' CLIPTextModel returns, as far as the reference reads it: attributes, and `out[0]` = last_hidden_state (train.py:644)."""

    def __init__(self, last_hidden_state, pooler_output, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states

    def __getitem__(self, i):
        return tuple(v for v in (self.last_hidden_state, self.pooler_output, self.hidden_states) if v is not None)[i]


class AbstractEncoder(nn.Module):
    def encode(self, *args, **kwargs):
        raise NotImplementedError


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])
        # checkpoints written by older transformers carry the arange buffer `position_ids`: accepted and ignored
        self._register_load_state_dict_pre_hook(self._drop_position_ids)

    @staticmethod
    def _drop_position_ids(state_dict, prefix, *_):
        state_dict.pop(prefix + "position_ids", None)


class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)


class _MLP(nn.Module):
    def __init__(self, C, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, I), nn.Linear(I, C)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.self_attn = _Attention(C)
        self.layer_norm1 = nn.LayerNorm(C, eps=eps)
        self.mlp = _MLP(C, cfg["intermediate_size"])
        self.layer_norm2 = nn.LayerNorm(C, eps=eps)

    def packed(self):
        """bf16 weight images + fp32 biases / affine vectors of this layer, rebuilt when any of its 16 tensors changes."""
        a, m = self.self_attn, self.mlp
        if ops.cache_stale(self, "_pk", *self.parameters()):
            f = lambda t: t.detach().float().contiguous()
            self._pk = types.SimpleNamespace(
                wqkv=torch.cat([ops.pack_linear(l.weight) for l in (a.q_proj, a.k_proj, a.v_proj)], 0).contiguous(),   # q | k | v packed once
                bqkv=torch.cat([f(l.bias) for l in (a.q_proj, a.k_proj, a.v_proj)], 0).contiguous(),
                wo=ops.pack_linear(a.out_proj.weight), bo=f(a.out_proj.bias),
                w1=ops.pack_linear(m.fc1.weight), b1=f(m.fc1.bias), w2=ops.pack_linear(m.fc2.weight), b2=f(m.fc2.bias),
                g1=f(self.layer_norm1.weight), e1=f(self.layer_norm1.bias), g2=f(self.layer_norm2.weight), e2=f(self.layer_norm2.bias))
        return self._pk


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg["num_hidden_layers"])])


class _TextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])


class CLIPTextTower(nn.Module):
    """`FrozenCLIPEmbedder.transformer`: transformers' CLIPTextModel (text_model.{embeddings, encoder.layers, final_layer_norm}) on HIP."""

    def __init__(self, config=None):
        super().__init__()
        cfg = dict(CLIP_VIT_L_TEXT)
        cfg.update(config or {})
        C, H = cfg["hidden_size"], cfg["num_attention_heads"]
        if C % H or C // H not in (32, 64):
            raise ValueError(f"CLIPTextTower: head_dim {C}/{H} is not covered by the causal attention kernel (32 or 64)")
        if cfg["max_position_embeddings"] > 128:
            raise ValueError("CLIPTextTower: the causal attention kernel covers at most 128 positions")
        if cfg["hidden_act"] not in _ACTS:
            raise ValueError(f"CLIPTextTower: hidden_act {cfg['hidden_act']!r} (supported: {sorted(_ACTS)})")
        self.config = cfg
        self.text_model = _TextTransformer(cfg)
        self._ws = {}

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    # ---- caches ---------------------------------------------------------------------------------------------------------------
    def _tables(self):
        e, n = self.text_model.embeddings, self.text_model.final_layer_norm
        if ops.cache_stale(self, "_pk", e.token_embedding.weight, e.position_embedding.weight, n.weight, n.bias):
            self._pk = types.SimpleNamespace(tok=e.token_embedding.weight.detach().to(BF16).contiguous(),
                                             pos=e.position_embedding.weight.detach().to(BF16).contiguous(),
                                             g=n.weight.detach().float().contiguous(), e=n.bias.detach().float().contiguous())
        return self._pk

    def weights_token(self):
        """Changes whenever any parameter of the tower does (callers cache encodings against it)."""
        return ops.weights_token(*self.parameters())

    def _workspace(self, B, N, dev):
        key = (B, N, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            cfg = self.config
            M, C, I, L = B * N, cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
            e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
            ws = self._ws[key] = types.SimpleNamespace(
                ids=torch.zeros(B, N, dtype=torch.int64, device=dev), hs=[e(M, C) for _ in range(L + 1)], h=e(M, C), qkv=e(M, 3 * C),
                att=e(M, C), mid=e(M, C), u=e(M, I, dt=torch.float32), act=e(M, I), z=e(M, C), pooled=e(B, C))
        return ws

    # ---- the tower ------------------------------------------------------------------------------------------------------------
    def _ids_on_device(self, ids):
        """ids -> (device id tensor, workspace).  Host ids (list / CPU tensor: what a tokenizer returns) are range-checked HERE, before any
        copy, and then copied into the workspace's static buffer; device ids are used in place and never read back (the embedding kernel
        clamps them into the table)."""
        if isinstance(ids, torch.Tensor) and ids.is_cuda:
            if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or not ids.is_contiguous():
                raise TypeError(f"input_ids: expected a contiguous int32 / int64 [B, N] tensor, got {ids.dtype} {tuple(ids.shape)}")
            host = None
        else:
            host = torch.as_tensor(ids).to(torch.int64)
            if host.dim() != 2 or host.numel() == 0:
                raise ValueError(f"input_ids: expected [B, N] token ids, got shape {tuple(host.shape)}")
            lo, hi, V = int(host.min()), int(host.max()), self.config["vocab_size"]
            if lo < 0 or hi >= V:
                raise ValueError(f"input_ids: token id {lo if lo < 0 else hi} is outside the vocabulary [0, {V})")
        B, N = (ids if host is None else host).shape
        if N > self.config["max_position_embeddings"]:
            raise ValueError(f"input_ids: {N} tokens, the position table has {self.config['max_position_embeddings']}")
        if self.device.type != "cuda":
            raise ValueError("CLIPTextTower: the tower runs on the GPU only (anyedit_amd has no CPU path); move it with .to('cuda')")
        ws = self._workspace(B, N, self.device)
        if host is None:
            return ids, ws
        ws.ids.copy_(host)
        return ws.ids, ws

    @torch.no_grad()
    def run(self, ids, n_layers=None):
        """Embeds `ids` and runs the first `n_layers` layers (all by default); returns (device ids, workspace) with `ws.hs[0 .. n_layers]`
        filled: hs[0] the embeddings, hs[i] the residual stream after layer i (transformers' `hidden_states`, no final LayerNorm)."""
        cfg = self.config
        ids, ws = self._ids_on_device(ids)
        B, N = ids.shape
        C, H = cfg["hidden_size"], cfg["num_attention_heads"]
        D, eps, act = C // H, cfg["layer_norm_eps"], _ACTS[cfg["hidden_act"]]
        L = cfg["num_hidden_layers"] if n_layers is None else n_layers
        t = self._tables()
        hs = ws.hs
        ops.clip_embed(ids, t.tok, t.pos, out=hs[0])                                               # bf16: embedding sum
        qkv = ws.qkv
        strides = (N * 3 * C, D, 3 * C)
        for i in range(L):
            p = self.text_model.encoder.layers[i].packed()
            ops.layernorm(hs[i], p.g1, p.e1, eps, out=ws.h)                                        # bf16: LayerNorm1 output (not folded: the fold covers K = 320 only)
            ops.gemm(ws.h, p.wqkv, p.bqkv, out=qkv)                                                # bf16: packed q | k | v
            ops.attention_causal_short(qkv, qkv[:, C:], qkv[:, 2 * C:], B, H, N, D, D ** -0.5, strides, strides, strides, out=ws.att)   # bf16: attention output
            ops.gemm(ws.att, p.wo, p.bo, residual=hs[i], out=ws.mid)                               # bf16: residual stream after the attention add
            ops.layernorm(ws.mid, p.g2, p.e2, eps, out=ws.h)                                       # bf16: LayerNorm2 output
            ops.gemm(ws.h, p.w1, None, out_f32=True, out=ws.u)                                     # fp32: fc1 product (bias and activation follow in fp32)
            ops.bias_act(ws.u, p.b1, act, out=ws.act)                                              # bf16: activated hidden values
            ops.gemm(ws.act, p.w2, p.b2, residual=ws.mid, out=hs[i + 1])                           # bf16: residual stream after the MLP add
        return ids, ws

    def final_norm(self, ws, index, B, N):
        """final_layer_norm(hidden_states[index]) -> the workspace's static [B, N, C] output."""
        t = self._tables()
        ops.layernorm(ws.hs[index], t.g, t.e, self.config["layer_norm_eps"], out=ws.z)             # bf16: final LayerNorm output
        return ws.z.view(B, N, -1)

    def forward(self, input_ids, output_hidden_states=False):
        """transformers' call: returns a `CLIPTextOutput` with last_hidden_state [B, N, C], pooler_output [B, C] and (on request) hidden_states, all
        bf16 views of the static workspace of this [B, N] (valid until the next call of that shape)."""
        ids, ws = self.run(input_ids)
        B, N = ids.shape
        last = self.final_norm(ws, self.config["num_hidden_layers"], B, N)
        pooled = ops.clip_pool_eos(ids, ws.z, self.config["eos_token_id"], out=ws.pooled)
        return CLIPTextOutput(last, pooled, tuple(h.view(B, N, -1) for h in ws.hs) if output_hidden_states else None)


class FrozenCLIPEmbedder(AbstractEncoder):
    """Uses the CLIP transformer encoder for text (modules.py:107-150), on the HIP path.  `tokenizer`: any object with the Hugging Face
    call signature; `config`: overrides of `CLIP_VIT_L_TEXT`.  `version` is only ever looked at as a LOCAL directory."""
    LAYERS = ["last", "pooled", "hidden"]

    def __init__(self, version="openai/clip-vit-large-patch14", device="cuda", max_length=77, freeze=True, layer="last", layer_idx=None,
                 tokenizer=None, config=None):
        super().__init__()
        assert layer in self.LAYERS
        self.transformer = CLIPTextTower(config)
        if tokenizer is None and isinstance(version, str) and os.path.isdir(version):
            from transformers import CLIPTokenizer
            tokenizer = CLIPTokenizer.from_pretrained(version, local_files_only=True)
        self.tokenizer = tokenizer
        self.version = version
        self.device = device
        self.max_length = max_length
        if freeze:
            self.freeze()
        self.layer = layer
        self.layer_idx = layer_idx
        if layer == "hidden":
            assert layer_idx is not None
            assert 0 <= abs(layer_idx) <= self.transformer.config["num_hidden_layers"]

    def freeze(self):
        self.transformer = self.transformer.eval()
        for param in self.parameters():
            param.requires_grad = False

    def _need_tokenizer(self):
        if self.tokenizer is None:
            raise ValueError(f"FrozenCLIPEmbedder has no tokenizer: pass tokenizer=<object with the Hugging Face call signature>, or a local "
                             f"directory as version= (got {self.version!r}, which is not one; nothing is ever downloaded).  "
                             f"encode_ids(input_ids) works without a tokenizer.")
        return self.tokenizer

    @torch.no_grad()
    def encode_ids(self, ids):
        """[B, N] token ids (N <= 77; list, CPU tensor or GPU tensor) -> the conditioning `layer` selects: "last" [B, N, C], "hidden" [B, N, C]
        (hidden_states[layer_idx], no final LayerNorm), "pooled" [B, 1, C]; bf16.

        Host ids are range-checked (ValueError) before any copy.  Ids already on the GPU are NOT read back — that would be a host
        synchronisation — so an id outside the vocabulary is clamped into the embedding table by the kernel instead of being reported.
        The result is a view of this shape's static buffer (no allocation after the first call, capturable in a graph): it is overwritten
        by the next call with the same [B, N] — `.clone()` it to keep it; `forward` / `encode` do."""
        tw = self.transformer
        L = tw.config["num_hidden_layers"]
        if self.layer == "hidden":
            idx = self.layer_idx if self.layer_idx >= 0 else L + 1 + self.layer_idx
            ids_d, ws = tw.run(ids, n_layers=idx)
            return ws.hs[idx].view(ids_d.shape[0], ids_d.shape[1], -1)
        ids_d, ws = tw.run(ids)
        B, N = ids_d.shape
        z = tw.final_norm(ws, L, B, N)
        if self.layer == "last":
            return z
        return ops.clip_pool_eos(ids_d, ws.z, tw.config["eos_token_id"], out=ws.pooled)[:, None, :]

    def forward(self, text):
        tok = self._need_tokenizer()
        batch_encoding = tok(text, truncation=True, max_length=self.max_length, return_length=True,
                             return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        return self.encode_ids(batch_encoding["input_ids"]).clone()

    def encode(self, text):
        return self(text)


def __getattr__(name):
    """`ldm.modules.encoders.modules.FrozenDinoV2Encoder` (anydoor.yaml's cond_stage_config target; modules.py:279-315) lives in dino_vision.py,
    which imports this module: resolved on first use."""
    if name == "FrozenDinoV2Encoder":
        from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder
        return FrozenDinoV2Encoder
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
