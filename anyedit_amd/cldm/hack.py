"""Mirror of AnyEdit_Collection/other_modules/cldm/hack.py (:11-68) — the run-time swap points the AnyDoor tool calls before building
its model (`disable_verbosity()`, `enable_sliced_attention()`, `hack_everything()`).

The reference's `enable_sliced_attention` monkey-patches `CrossAttention.forward` with a per-head loop so the [B*h, N, N] logits never
exist at once.  On this path CrossAttention is already the fused flash-style HIP kernel (no logits tensor at all), so the call is
accepted and changes nothing.

`hack_everything(clip_skip)` installs the reference's long-prompt forward (:32-68) on this package's `FrozenCLIPEmbedder`: the prompt is
tokenized without truncation, cut into three 75-token chunks, each framed as [BOS] chunk [EOS] and padded to 77, the 3B rows go through
the HIP text tower in one batch and come back as [B, 231, C].  `clip_skip > 1` takes `final_layer_norm(hidden_states[-clip_skip])`
instead of the last hidden state.
"""
import torch


def disable_verbosity():
    try:
        from transformers import logging
        logging.set_verbosity_error()
    except ImportError:  # transformers is optional: the tower itself does not use it
        pass
    print('logging improved.')
    return


def enable_sliced_attention():
    print('Enabled sliced_attention. (no-op: attention is the fused HIP kernel, the logits tensor is never materialised)')
    return


def hack_everything(clip_skip=0):
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    disable_verbosity()
    FrozenCLIPEmbedder.forward = _hacked_clip_forward
    FrozenCLIPEmbedder.clip_skip = clip_skip
    print('Enabled clip hacks.')
    return


def frame_chunks(raw_tokens_list, bos, eos, pad, chunk=75, chunks=3):
    """hack.py:47-60 (host logic): every raw token list -> `chunks` rows of chunk + 2 ids, [BOS] + tokens[chunk*i : chunk*(i+1)] + [EOS]
    padded with PAD; tokens beyond chunk * chunks are dropped.  Returns a [len(list), chunks, chunk + 2] nested list."""
    out = []
    for raw in raw_tokens_list:
        rows = []
        for i in range(chunks):
            row = [bos] + list(raw[chunk * i: chunk * (i + 1)]) + [eos]
            rows.append(row + [pad] * (chunk + 2 - len(row)))
        out.append(rows)
    return out


@torch.no_grad()
def encode_framed(embedder, tokens, clip_skip=0):
    """hack.py:40-45, 62-68: [B, 3, 77] framed ids -> [B, 231, C] through the HIP tower (one batch of 3B rows)."""
    ids = torch.as_tensor(tokens, dtype=torch.int64)
    B, F, N = ids.shape
    tw = embedder.transformer
    L = tw.config["num_hidden_layers"]
    index = L + 1 - clip_skip if clip_skip > 1 else L
    if not 0 <= index <= L:
        raise ValueError(f"clip_skip {clip_skip} reaches past the {L + 1} hidden states of the tower")
    ids_d, ws = tw.run(ids.reshape(B * F, N), n_layers=index)
    return tw.final_norm(ws, index, B * F, N).reshape(B, F * N, -1).clone()


def _hacked_clip_forward(self, text):
    tok = self._need_tokenizer()
    raw_tokens_list = tok(text, truncation=False, add_special_tokens=False)["input_ids"]
    tokens = frame_chunks(raw_tokens_list, tok.bos_token_id, tok.eos_token_id, tok.pad_token_id)
    return encode_framed(self, tokens, getattr(self, "clip_skip", 0))
