"""GroundingDINO/groundingdino/models/GroundingDINO/bertwarper.py on the HIP path: the BERT text encoder GroundingDINO reads its caption with,
`BertModelWarper`, and the two sub-sentence mask generators (:180-273).

`BertModel` is transformers' BertModel (absolute positions, post-LN, erf-GELU, tanh pooler) restated over the library, under Hugging Face's
state-dict keys (`embeddings.*`, `encoder.layer.N.*`, `pooler.dense.*`), so the `bert.*` entries of a GroundingDINO checkpoint load unchanged:

    x0 = LayerNorm(word[ids] + position[position_ids] + token_type[type_ids])                    ops.bert_embed_ln           # bf16
    per layer:
      q|k|v = x Wqkv^T + b            (ONE [3C, C] GEMM)                                         ops.gemm                    # bf16
      a     = softmax(d^-0.5 q k^T over the allowed keys) v                                      ops.attention_span_short    # bf16
      y     = LayerNorm(x + a Wo^T + bo)                                                         ops.gemm (residual), ops.layernorm
      u     = gelu(y W1^T + b1)       (fp32 product, bias and GELU in fp32)                      ops.gemm (out_f32), ops.bias_act
      x'    = LayerNorm(y + u W2^T + b2)                                                         ops.gemm (residual), ops.layernorm
    pooler_output = tanh(x_L[:, 0] Wp^T + bp)   (fp32, only when asked for)                      ops.gemm (out_f32), torch.tanh on [B, C]

Every activation stored between two launches is bf16; the points are marked `# bf16:` below and tests/bert_ref.py rounds at exactly those points
for its control.

Attention routes.  GroundingDINO's sub-sentence masks are block-diagonal: every query attends ONE contiguous key range.  `key_spans` (int32
[B, N, 2], what `ops.gdino_text_spans` writes) takes the product's route, `ops.attention_span_short`, which reads two integers per query where a
mask kernel would read a [B*H, N, N] byte array the caller had to expand over 12 heads first.  No mask at all is the span [0, N).  A 2-D padding
mask or a general 3-D mask goes to `ops.attention_masked_short` with the mask expanded over heads (the general route, not the product's).

One call on a given [B, N] makes no allocation and no host synchronisation after the first, runs on the current stream only, and may be captured
in a graph: its buffers (the returned tensors included) are static per shape and are overwritten by the next call of that shape.
"""
import types

import torch
import torch.nn as nn

from anyedit_amd import ops

BF16 = torch.bfloat16

# bert-base-uncased (get_tokenlizer.py: the text_encoder_type of every released GroundingDINO)
BERT_BASE = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                 position_embedding_type="absolute", is_decoder=False)
MAX_TOKENS = ops.TEXT_SPANS_MAX_N


def _f32(t):
    return t.detach().float().contiguous()


class BertOutput:
    """What transformers' BertModel returns, as far as the reference reads it: attributes, `out["last_hidden_state"]` (groundingdino.py:265)
    and `out[0]` / `out[1]`."""

    def __init__(self, last_hidden_state, pooler_output=None, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return (self.last_hidden_state, self.pooler_output, self.hidden_states)[i]


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C = cfg["hidden_size"]
        self.word_embeddings = nn.Embedding(cfg["vocab_size"], C)
        self.position_embeddings = nn.Embedding(cfg["max_position_embeddings"], C)
        self.token_type_embeddings = nn.Embedding(cfg["type_vocab_size"], C)
        self.LayerNorm = nn.LayerNorm(C, eps=cfg["layer_norm_eps"])
        # checkpoints written by older transformers carry the arange buffer `position_ids` (and some `token_type_ids`): accepted and ignored
        self._register_load_state_dict_pre_hook(self._drop_buffers)

    @staticmethod
    def _drop_buffers(state_dict, prefix, *_):
        state_dict.pop(prefix + "position_ids", None)
        state_dict.pop(prefix + "token_type_ids", None)


class _SelfAttention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)


class _Output(nn.Module):
    def __init__(self, cin, C, eps):
        super().__init__()
        self.dense = nn.Linear(cin, C)
        self.LayerNorm = nn.LayerNorm(C, eps=eps)


class _Attention(nn.Module):
    def __init__(self, C, eps):
        super().__init__()
        self.self = _SelfAttention(C)
        self.output = _Output(C, C, eps)


class _Intermediate(nn.Module):
    def __init__(self, C, I):
        super().__init__()
        self.dense = nn.Linear(C, I)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C, I, eps = cfg["hidden_size"], cfg["intermediate_size"], cfg["layer_norm_eps"]
        self.attention = _Attention(C, eps)
        self.intermediate = _Intermediate(C, I)
        self.output = _Output(I, C, eps)

    def packed(self):
        """bf16 weight images + fp32 biases / affine vectors of this layer, rebuilt when any of its 16 tensors changes."""
        if ops.cache_stale(self, "_pk", *self.parameters()):
            s, ao, o = self.attention.self, self.attention.output, self.output
            self._pk = types.SimpleNamespace(
                wqkv=torch.cat([ops.pack_linear(l.weight) for l in (s.query, s.key, s.value)], 0).contiguous(),   # q | k | v packed once
                bqkv=torch.cat([_f32(l.bias) for l in (s.query, s.key, s.value)], 0).contiguous(),
                wo=ops.pack_linear(ao.dense.weight), bo=_f32(ao.dense.bias), g1=_f32(ao.LayerNorm.weight), e1=_f32(ao.LayerNorm.bias),
                w1=ops.pack_linear(self.intermediate.dense.weight), b1=_f32(self.intermediate.dense.bias),
                w2=ops.pack_linear(o.dense.weight), b2=_f32(o.dense.bias), g2=_f32(o.LayerNorm.weight), e2=_f32(o.LayerNorm.bias))
        return self._pk


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(cfg) for _ in range(cfg["num_hidden_layers"])])


class _Pooler(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.dense = nn.Linear(C, C)


class BertModel(nn.Module):
    """transformers' BertModel (encoder only, with pooler) on HIP.  `config`: a dict (or keywords) over `BERT_BASE`."""

    def __init__(self, config=None, **kw):
        super().__init__()
        cfg = dict(BERT_BASE)
        cfg.update(dict(config) if config is not None else {})
        cfg.update(kw)
        C, H = cfg["hidden_size"], cfg["num_attention_heads"]
        if cfg.get("is_decoder"):
            raise NotImplementedError("BertModel: is_decoder=True is not built (no causal mask, no cross-attention, no key/value cache)")
        if cfg["hidden_act"] != "gelu":
            raise NotImplementedError(f"BertModel: hidden_act {cfg['hidden_act']!r} is not built (supported: 'gelu', the erf form)")
        if cfg.get("position_embedding_type", "absolute") != "absolute":
            raise NotImplementedError(f"BertModel: position_embedding_type {cfg['position_embedding_type']!r} is not built (supported: 'absolute')")
        if C % H or C // H != 64:
            raise ValueError(f"BertModel: head_dim {C}/{H} must be 64 (ae_attn_span_short_bf16)")
        if C % 8 or cfg["intermediate_size"] % 8 or C > ops.BERT_EMBED_MAX_C:
            raise ValueError(f"BertModel: hidden_size {C} and intermediate_size {cfg['intermediate_size']} must be multiples of 8, hidden_size at most "
                             f"{ops.BERT_EMBED_MAX_C}")
        self.config = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.pooler = _Pooler(C)
        self._ws = {}

    @property
    def device(self):
        return self.pooler.dense.weight.device

    def _dropouts(self):
        return (self.config.get("hidden_dropout_prob", 0.0), self.config.get("attention_probs_dropout_prob", 0.0))

    # ---- caches ---------------------------------------------------------------------------------------------------------------
    def _tables(self):
        e, p = self.embeddings, self.pooler.dense
        if ops.cache_stale(self, "_pk", *e.parameters(), p.weight, p.bias):
            self._pk = types.SimpleNamespace(word=e.word_embeddings.weight.detach().to(BF16).contiguous(),
                                             pos=e.position_embeddings.weight.detach().to(BF16).contiguous(),
                                             typ=e.token_type_embeddings.weight.detach().to(BF16).contiguous(),
                                             g=_f32(e.LayerNorm.weight), e=_f32(e.LayerNorm.bias), wp=ops.pack_linear(p.weight), bp=_f32(p.bias))
        return self._pk

    def _workspace(self, B, N, dev):
        key = (B, N, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            cfg = self.config
            M, C, I, L = B * N, cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
            e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
            idx = lambda: torch.zeros(B, N, dtype=torch.int64, device=dev)
            full = torch.zeros(B, N, 2, dtype=torch.int32, device=dev)
            full[..., 1] = N
            ws = self._ws[key] = types.SimpleNamespace(
                ids=idx(), pids=idx(), tids=idx(), spans=torch.zeros(B, N, 2, dtype=torch.int32, device=dev), full=full, mask=None,
                hs=[e(M, C) for _ in range(L + 1)], qkv=e(M, 3 * C), att=e(M, C), mid=e(M, C), y=e(M, C), u=e(M, I, dt=torch.float32), act=e(M, I),
                pool=e(B, C, dt=torch.float32), pooled=e(B, C, dt=torch.float32))
        return ws

    # ---- inputs ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _index(t, buf, name, B, N):
        """An index tensor as the kernels read it: an int64 contiguous GPU tensor is used in place (never read back); anything else (a list, a CPU
        tensor — what a tokenizer returns —, another integer type) is copied into the workspace's static buffer."""
        if t is None:
            return None
        t = torch.as_tensor(t)
        if tuple(t.shape) != (B, N):
            raise ValueError(f"BertModel: {name} of shape {tuple(t.shape)}; expected {(B, N)}")
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f"BertModel: {name} must hold integers, got {t.dtype}")
        if t.is_cuda and t.dtype == torch.int64 and t.is_contiguous():
            return t
        buf.copy_(t)
        return buf

    def _check_host_ids(self, ids):
        """Host ids are range-checked here, before any copy; device ids are never read back (the embedding kernel clamps them into the table)."""
        if not (isinstance(ids, torch.Tensor) and ids.is_cuda):
            host = torch.as_tensor(ids)
            if host.dim() != 2 or host.numel() == 0:
                raise ValueError(f"BertModel: input_ids: expected [B, N] token ids, got shape {tuple(host.shape)}")
            lo, hi, V = int(host.min()), int(host.max()), self.config["vocab_size"]
            if lo < 0 or hi >= V:
                raise ValueError(f"BertModel: input_ids: token id {lo if lo < 0 else hi} is outside the vocabulary [0, {V})")
            return host
        if ids.dim() != 2:
            raise ValueError(f"BertModel: input_ids: expected [B, N] token ids, got shape {tuple(ids.shape)}")
        return ids

    def _head_mask(self, ws, m, B, H, N, dev):
        """2-D [B, N] (keys) / 3-D [B, N, N] / 4-D [B, 1, N, N] mask, non-zero = allowed -> the workspace's uint8 [B*H, N, N]."""
        m = torch.as_tensor(m)
        if m.dim() == 2 and tuple(m.shape) == (B, N):
            src = m.view(B, 1, 1, N)
        elif m.dim() == 3 and tuple(m.shape) == (B, N, N):
            src = m.view(B, 1, N, N)
        elif m.dim() == 4 and tuple(m.shape) == (B, 1, N, N):
            src = m
        else:
            raise ValueError(f"BertModel: attention_mask of shape {tuple(m.shape)}; expected {(B, N)}, {(B, N, N)} or {(B, 1, N, N)}")
        if ws.mask is None:
            ws.mask = torch.zeros(B, H, N, N, dtype=torch.bool, device=dev)
        ws.mask.copy_(src.to(dev) if src.device != dev else src)            # converts (non-zero = True) and broadcasts over heads and queries
        return ws.mask.view(B * H, N, N)

    # ---- the encoder ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None, inputs_embeds=None,
                encoder_hidden_states=None, encoder_attention_mask=None, past_key_values=None, use_cache=None, output_attentions=None,
                output_hidden_states=False, return_dict=None, key_spans=None, output_pooler=True):
        """transformers' call.  input_ids [B, N] (N <= 256); attention_mask None, [B, N], [B, N, N] or [B, 1, N, N] (non-zero = the key is
        allowed; CONTRACT: every query allows a key); key_spans int32 [B, N, 2] (`ops.gdino_text_spans`; CONTRACT 0 <= lo < hi <= N) selects
        the span kernel and excludes attention_mask.  Returns a `BertOutput`: last_hidden_state [B, N, C] bf16, pooler_output [B, C] fp32
        (None with output_pooler=False), hidden_states (L + 1 tensors, on request) — views of this shape's static workspace."""
        from anyedit_amd.groundingdino.fuse_modules import require_inference
        for v, n in ((head_mask, "head_mask"), (inputs_embeds, "inputs_embeds"), (past_key_values, "past_key_values"),
                     (encoder_hidden_states, "encoder_hidden_states"), (encoder_attention_mask, "encoder_attention_mask")):
            if v is not None:
                raise NotImplementedError(f"BertModel: {n} is not built (the reference never passes it)")
        if output_attentions:
            raise NotImplementedError("BertModel: output_attentions is not built (no probability matrix is ever stored)")
        if use_cache:
            raise NotImplementedError("BertModel: use_cache is not built (encoder only)")
        if input_ids is None:
            raise ValueError("BertModel: input_ids is required")
        if key_spans is not None and attention_mask is not None:
            raise ValueError("BertModel: pass key_spans or attention_mask, not both")
        require_inference(self, self._dropouts())
        cfg = self.config
        dev = self.device
        input_ids = self._check_host_ids(input_ids)
        if dev.type != "cuda":
            raise ValueError("BertModel: the encoder runs on the GPU only (anyedit_amd has no CPU path); move it with .to('cuda')")
        B, N = input_ids.shape
        if not 1 <= N <= MAX_TOKENS:
            raise ValueError(f"BertModel: {N} tokens; the attention kernels take between 1 and {MAX_TOKENS}")
        if position_ids is None and N > cfg["max_position_embeddings"]:
            raise ValueError(f"BertModel: {N} tokens, the position table has {cfg['max_position_embeddings']} rows")
        C, H, L, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["layer_norm_eps"]
        D = C // H
        ws = self._workspace(B, N, dev)
        ids = self._index(input_ids, ws.ids, "input_ids", B, N)
        pids = self._index(position_ids, ws.pids, "position_ids", B, N)
        tids = self._index(token_type_ids, ws.tids, "token_type_ids", B, N)
        spans = mask = None
        if key_spans is not None:
            if not (isinstance(key_spans, torch.Tensor) and key_spans.is_cuda and key_spans.dtype == torch.int32 and key_spans.is_contiguous()
                    and tuple(key_spans.shape) == (B, N, 2)):
                ws.spans.copy_(torch.as_tensor(key_spans).reshape(B, N, 2))
                key_spans = ws.spans
            spans = key_spans
        elif attention_mask is None:
            spans = ws.full
        else:
            mask = self._head_mask(ws, attention_mask, B, H, N, dev)

        t = self._tables()
        hs = ws.hs
        ops.bert_embed_ln(ids, t.word, t.pos, t.typ, t.g, t.e, eps, position_ids=pids, type_ids=tids, out=hs[0])     # bf16: embeddings after their LayerNorm
        qkv = ws.qkv
        strides = (N * 3 * C, D, 3 * C)
        for i in range(L):
            p = self.encoder.layer[i].packed()
            ops.gemm(hs[i], p.wqkv, p.bqkv, out=qkv)                                               # bf16: packed q | k | v
            if spans is not None:
                ops.attention_span_short(qkv, qkv[:, C:], qkv[:, 2 * C:], spans, B, H, N, D, D ** -0.5, strides, strides, strides, out=ws.att)   # bf16: attention output
            else:
                ops.attention_masked_short(qkv, qkv[:, C:], qkv[:, 2 * C:], mask, B, H, N, D, D ** -0.5, strides, strides, strides, out=ws.att)  # bf16: attention output
            ops.gemm(ws.att, p.wo, p.bo, residual=hs[i], out=ws.mid)                               # bf16: x + attention projection
            ops.layernorm(ws.mid, p.g1, p.e1, eps, out=ws.y)                                       # bf16: attention.output.LayerNorm
            ops.gemm(ws.y, p.w1, None, out_f32=True, out=ws.u)                                     # fp32: intermediate product (bias and GELU follow in fp32)
            ops.bias_act(ws.u, p.b1, ops.ACT_GELU, out=ws.act)                                     # bf16: activated hidden values
            ops.gemm(ws.act, p.w2, p.b2, residual=ws.y, out=ws.mid)                                # bf16: y + output projection
            ops.layernorm(ws.mid, p.g2, p.e2, eps, out=hs[i + 1])                                  # bf16: output.LayerNorm = hidden_states[i + 1]
        pooled = None
        if output_pooler:
            ops.gemm(hs[L].view(B, N * C)[:, :C], t.wp, t.bp, out_f32=True, out=ws.pool)           # fp32: pooler product + bias on row 0 of every sample
            pooled = torch.tanh(ws.pool, out=ws.pooled)                                            # fp32: pooler_output
        view = lambda h: h.view(B, N, C)
        return BertOutput(view(hs[L]), pooled, tuple(view(h) for h in hs) if output_hidden_states else None)


class BertModelWarper(nn.Module):
    """bertwarper.py:17-166: the reference's wrapper shares the wrapped model's submodules and re-implements its forward so that a 3-D
    [B, N, N] attention mask passes.  `BertModel.forward` takes that mask already; the wrapper keeps the names (`embeddings`, `encoder`,
    `pooler`, `config`: the `bert.*` keys of a checkpoint) and forwards."""

    def __init__(self, bert_model):
        super().__init__()
        if not isinstance(bert_model, BertModel):
            raise TypeError(f"BertModelWarper: expected anyedit_amd's BertModel, got {type(bert_model).__name__}")
        self.config = bert_model.config
        self.embeddings = bert_model.embeddings
        self.encoder = bert_model.encoder
        self.pooler = bert_model.pooler
        self.__dict__["_model"] = bert_model      # not a submodule: its parameters are registered once, through the three above

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, **kw):
        return self.__dict__["_model"](input_ids=input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids, **kw)

    def train(self, mode=True):
        super().train(mode)
        self.__dict__["_model"].training = mode   # the wrapped model shares the submodules; its own flag follows the wrapper's
        return self


# ---- sub-sentence masks (bertwarper.py:180-273) ---------------------------------------------------------------------------------------------
def _spans_for(tokenized, special_tokens_list):
    ids = torch.as_tensor(tokenized["input_ids"])
    if ids.dim() != 2:
        raise ValueError(f"generate_masks_with_special_tokens: input_ids of shape {tuple(ids.shape)}; expected [bs, num_token]")
    if not ids.is_cuda:
        raise ValueError("generate_masks_with_special_tokens: input_ids must be on the GPU (anyedit_amd has no CPU path)")
    if ids.dtype not in (torch.int32, torch.int64):
        ids = ids.long()
    ids = ids.contiguous()
    return (ids,) + ops.gdino_text_spans(ids, list(special_tokens_list), want_mask=True)


def generate_masks_with_special_tokens(tokenized, special_tokens_list, tokenizer=None):
    """bertwarper.py:180-221 on `ops.gdino_text_spans`: returns (attention_mask bool [bs, N, N], position_ids long [bs, N]).  One launch, no
    host synchronisation.  CONTRACT (the reference's own: it does not reset `previous_col` per row): column 0 of every row is a special token."""
    _, _, pos, mask = _spans_for(tokenized, special_tokens_list)
    return mask, pos


def cate_to_token_masks(special, spans):
    """Host side of bertwarper.py:259-261: `special` bool [bs, N] (is the token a special one) and `spans` int [bs, N, 2], both on the host ->
    per sample a bool [phrases, N] tensor.  Every special token that is neither first nor last closes one phrase: a row that marks the tokens
    of its span without the special token itself (an empty row when two special tokens are adjacent, as in the reference)."""
    bs, N = special.shape
    out = []
    for b in range(bs):
        rows = []
        for e in torch.nonzero(special[b]).flatten().tolist():
            if e == 0 or e == N - 1:
                continue
            r = torch.zeros(N, dtype=torch.bool)
            r[int(spans[b, e, 0]):e] = True
            rows.append(r)
        out.append(torch.stack(rows, 0) if rows else torch.zeros(0, N, dtype=torch.bool))
    return out


def generate_masks_with_special_tokens_and_transfer_map(tokenized, special_tokens_list, tokenizer=None):
    """bertwarper.py:224-273: as above plus `cate_to_token_mask_list`, per sample a bool [phrases, N] tensor whose rows mark the tokens of one
    phrase each.  THIS VARIANT SYNCHRONISES: the ragged list is built on the host from one read-back of the spans (with the ids beside them) —
    the only host synchronisation of the text side; the product route, `GroundingDINOText.encode_tokenized`, does not call it."""
    ids, spans, pos, mask = _spans_for(tokenized, special_tokens_list)
    bs, N = ids.shape
    host = torch.cat([spans.view(bs, 2 * N).long(), ids.long()], 1).cpu()                      # the one read-back
    hspans, hids = host[:, :2 * N].view(bs, N, 2), host[:, 2 * N:]
    special = torch.zeros(bs, N, dtype=torch.bool)
    for s in special_tokens_list:
        special |= hids == int(s)
    return mask, pos, [m.to(mask.device) for m in cate_to_token_masks(special, hspans)]
