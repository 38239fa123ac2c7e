"""GroundingDINO/groundingdino/models/GroundingDINO/groundingdino.py:106-119 and :233-283 — the text side of the detector on the HIP path: a
caption goes in, the `text_dict` that `transformer.Transformer.forward` reads comes out.

    tokenized = tokenizer(captions, padding="longest")                                            host (the caller's tokenizer)
    spans, position_ids, text_self_attention_masks = sub-sentence rule(input_ids)                 ops.gdino_text_spans       (:237-243)
    truncation to max_text_len                                                                    copies into static buffers (:245-252)
    last_hidden_state = bert(input_ids, token_type_ids, position_ids, key_spans=spans)            bertwarper.BertModel       (:255-263)
    encoded_text = feat_map(last_hidden_state)                                                    ops.gemm                   (:265)      # bf16

`GroundingDINOText` holds `bert` and `feat_map` under the checkpoint's names; the model class that will hold the backbone, `input_proj` and
the transformer beside them is not built yet.  The tokenizer is an object the caller passes in: nothing here reaches for a network.

`encoded_text` is bf16, the dtype `Transformer.forward` turns its text rows into (`as_rows`), so no conversion launch sits between the two.
After the first call at a given (B, N) `encode_tokenized` makes no allocation and no host synchronisation when its inputs are already on the
GPU, runs on the current stream only (no parallel branches) and may be captured in a graph; the four returned tensors are static per shape.
"""
import types

import torch
import torch.nn as nn

from anyedit_amd import ops
from anyedit_amd.groundingdino.bertwarper import MAX_TOKENS, BertModel, BertModelWarper

BF16 = torch.bfloat16
SPECIAL_TOKENS = ["[CLS]", "[SEP]", ".", "?"]           # groundingdino.py:119


class GroundingDINOText(nn.Module):
    def __init__(self, bert_config=None, hidden_dim=256, tokenizer=None, max_text_len=256, sub_sentence_present=True, special_token_ids=None):
        """bert_config: dict over `bertwarper.BERT_BASE`; tokenizer: any object with the Hugging Face call signature and `convert_tokens_to_ids`
        (or pass `special_token_ids`, the ids of "[CLS]", "[SEP]", ".", "?", and call `encode_tokenized` yourself)."""
        super().__init__()
        if not 1 <= max_text_len <= MAX_TOKENS:
            raise ValueError(f"GroundingDINOText: max_text_len {max_text_len} outside [1, {MAX_TOKENS}]")
        if hidden_dim % 8:
            raise ValueError(f"GroundingDINOText: hidden_dim {hidden_dim} must be a multiple of 8")
        self.bert = BertModelWarper(BertModel(bert_config))
        self.feat_map = nn.Linear(self.bert.config["hidden_size"], hidden_dim, bias=True)
        nn.init.constant_(self.feat_map.bias.data, 0)
        nn.init.xavier_uniform_(self.feat_map.weight.data)
        self.hidden_dim = hidden_dim
        self.tokenizer = tokenizer
        self.max_text_len = max_text_len
        self.sub_sentence_present = sub_sentence_present
        if special_token_ids is None:
            if tokenizer is None:
                raise ValueError("GroundingDINOText: pass tokenizer= (an object with convert_tokens_to_ids) or special_token_ids=; nothing is ever downloaded")
            special_token_ids = tokenizer.convert_tokens_to_ids(SPECIAL_TOKENS)
        self.specical_tokens = [int(t) for t in special_token_ids]           # the reference's spelling
        if len(self.specical_tokens) > 8:
            raise ValueError("GroundingDINOText: at most 8 special token ids")
        self._ws = {}

    def _packed(self):
        f = self.feat_map
        if ops.cache_stale(self, "_pk", f.weight, f.bias):
            self._pk = types.SimpleNamespace(w=ops.pack_linear(f.weight), b=f.bias.detach().float().contiguous())
        return self._pk

    def _workspace(self, B, N0, N, dev):
        key = (B, N0, N, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev)
            ws = self._ws[key] = types.SimpleNamespace(
                ids=z(B, N0, dt=torch.int64), tids=z(B, N0, dt=torch.int64), amask=z(B, N0, dt=torch.bool), spans=z(B, N0, 2, dt=torch.int32),
                pos=z(B, N0, dt=torch.int64), mask=z(B, N0, N0, dt=torch.bool), enc=z(B, N, self.hidden_dim, dt=BF16))
            if N != N0:
                ws.ids_t, ws.tids_t, ws.amask_t = z(B, N, dt=torch.int64), z(B, N, dt=torch.int64), z(B, N, dt=torch.bool)
                ws.spans_t, ws.pos_t, ws.mask_t = z(B, N, 2, dt=torch.int32), z(B, N, dt=torch.int64), z(B, N, N, dt=torch.bool)
        return ws

    @staticmethod
    def _in(t, buf):
        """A GPU tensor of the buffer's dtype is used in place; anything else (a tokenizer's CPU tensors) is copied into the static buffer."""
        t = torch.as_tensor(t)
        if t.is_cuda and t.dtype == buf.dtype and t.is_contiguous() and t.device == buf.device:
            return t
        buf.copy_(t)
        return buf

    @torch.no_grad()
    def encode_tokenized(self, tokenized):
        """groundingdino.py:237-283.  tokenized: a mapping with `input_ids` [B, N0] and `attention_mask` [B, N0] (`token_type_ids` optional: zeros),
        on the host or the GPU, N0 <= 256, column 0 of every row a special token ([CLS]).  Returns the text_dict: `encoded_text` bf16
        [B, N, hidden_dim], `text_token_mask` bool [B, N], `position_ids` long [B, N], `text_self_attention_masks` bool [B, N, N], with
        N = min(N0, max_text_len); static per shape (overwritten by the next call of that shape)."""
        dev = self.feat_map.weight.device
        if dev.type != "cuda":
            raise ValueError("GroundingDINOText: the encoder runs on the GPU only (anyedit_amd has no CPU path); move it with .to('cuda')")
        ids = torch.as_tensor(tokenized["input_ids"])
        if ids.dim() != 2 or ids.numel() == 0:
            raise ValueError(f"GroundingDINOText: input_ids of shape {tuple(ids.shape)}; expected [B, N]")
        if not ids.is_cuda:
            self.bert.__dict__["_model"]._check_host_ids(ids)
        B, N0 = ids.shape
        if N0 > MAX_TOKENS:
            raise ValueError(f"GroundingDINOText: {N0} tokens; the sub-sentence rule runs on at most {MAX_TOKENS} (truncate the caption in the tokenizer)")
        N = min(N0, self.max_text_len)
        ws = self._workspace(B, N0, N, dev)
        ids = self._in(ids, ws.ids)
        amask = self._in(tokenized["attention_mask"], ws.amask)
        tt = tokenized.get("token_type_ids") if hasattr(tokenized, "get") else tokenized["token_type_ids"]
        tids = None if tt is None else self._in(tt, ws.tids)
        spans, pos, mask = ops.gdino_text_spans(ids, self.specical_tokens, spans=ws.spans, position_ids=ws.pos, dense_mask=ws.mask)   # :237-243
        if N != N0:                                                                    # :245-252
            ws.ids_t.copy_(ids[:, :N])
            ws.amask_t.copy_(amask[:, :N])
            ws.pos_t.copy_(pos[:, :N])
            ws.mask_t.copy_(mask[:, :N, :N])
            torch.clamp(spans[:, :N], max=N, out=ws.spans_t)                           # a span cut by the truncation keeps its keys below N
            ids, amask, pos, mask, spans = ws.ids_t, ws.amask_t, ws.pos_t, ws.mask_t, ws.spans_t
            if tids is not None:
                ws.tids_t.copy_(tids[:, :N])
                tids = ws.tids_t
        if self.sub_sentence_present:                                                  # :255-263
            out = self.bert(input_ids=ids, token_type_ids=tids, position_ids=pos, key_spans=spans, output_pooler=False)
        else:
            out = self.bert(input_ids=ids, token_type_ids=tids, attention_mask=amask, output_pooler=False)
        pk = self._packed()
        C = self.bert.config["hidden_size"]
        ops.gemm(out.last_hidden_state.view(B * N, C), pk.w, pk.b, out=ws.enc.view(B * N, self.hidden_dim))      # bf16: feat_map (:265)
        return {"encoded_text": ws.enc, "text_token_mask": amask, "position_ids": pos, "text_self_attention_masks": mask}

    def forward(self, captions):
        """captions: list of strings -> the text_dict (fresh tensors)."""
        if self.tokenizer is None:
            raise ValueError("GroundingDINOText has no tokenizer: pass tokenizer=<object with the Hugging Face call signature>, or tokenize "
                             "yourself and call encode_tokenized(tokenized); nothing is ever downloaded")
        tokenized = self.tokenizer(captions, padding="longest", return_tensors="pt")   # :234
        return {k: v.clone() for k, v in self.encode_tokenized(tokenized).items()}
