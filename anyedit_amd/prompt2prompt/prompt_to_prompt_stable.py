"""Mirror of AnyEdit_Collection/other_modules/prompt2prompt/prompt_to_prompt_stable.py (reference file:line cited per class) on the HIP attention
operators.  Names, constructor signatures and counting are the reference's; wherever the reference reads its module-level `tokenizer`, a
`tokenizer=` keyword is taken instead.

The batch is the reference's [uncond (P), cond (P)] (:108-109: only `attn[h // 2:]`, the conditional half, is controlled or stored); prompt 0 is the
base of prompts 1 .. P-1.  No attention_probs tensor is formed:
  * the store keeps, per place and in call order, ONE fp32 [P, N, Nk] buffer per cross-attention call with N <= 32^2: the SUM over heads (and, as
    the steps go by, over steps) of the probabilities, written by `ops.attention_p2p` straight into it, plus the call's head count.  step_store and
    between_steps' additions (:138-145) need no launches; get_average_attention / aggregate_attention divide by heads and steps on demand.  The
    stored maps are the post-edit ones, as in the reference (it stores a view and then writes the edit through it in place);
  * every cross-attention edit of the reference is P' = (P_base M) * c + P_own * d with, a = cross_replace_alpha[cur_step]:
    Replace (mapper, a, 1 - a); Refine (one-hot gather of the mapper, alphas a, 1 - alphas a); Reweight (identity, eq a, 1 - a); Reweight over a
    previous controller (M0, c0, d0): (M0, c0 eq a, d0 eq a + 1 - a).  Where an edit is live (c != 0 or d != 1 somewhere) the conditional half is
    ONE `ops.attention_p2p` launch (output and store), followed by the plain `ops.attention` on the unconditional half and the base (whose rows it
    overwrites: prompt 0 keeps the bits of a run without a controller); everywhere else (AttentionStore,
    EmptyControl, a closed gate) the output is `core()`, bit-identical to a model without a controller, and the store a store-only launch.  An
    edited call does not combine with an attention adapter (the expert key/value segment of `core`): `core` is not consulted for it;
  * self-attention replacement (:177-181) is two stride-only `ops.attention` launches on the packed projection: the unconditional half and the
    base as they are, the edited samples with batch stride 0 on q and k (the base's) and their own v.  Above 16^2 tokens the call is `core()`.

Not built: storing self-attention maps (their only reader is show_self_attention_comp, a visualisation), show_cross_attention and the image
helpers, run_and_display, LOW_RESOURCE, the diffusers registration, graph capture across steps."""
import abc

import numpy as np
import torch

from anyedit_amd import ops
from . import ptp_utils, seq_aligner

MAX_NUM_WORDS = 77
LOW_RESOURCE = False


def _need(tokenizer, who):
    if tokenizer is None:
        raise ValueError(f"{who}: pass tokenizer= (this package reads no global tokenizer and loads none)")
    return tokenizer


class LocalBlend:
    """:58-85.  __call__(x_t, attention_store): the maps down_cross[2:4] + up_cross[:3] summed over each prompt's words, pooled, resized, normalised
    and thresholded into one mask, x_t[1] blended towards x_t[0] outside it: one `ops.p2p_local_blend` launch, no read-back."""

    def __init__(self, prompts, words, threshold=.3, tokenizer=None):
        tokenizer = _need(tokenizer, "LocalBlend")
        alpha_layers = torch.zeros(len(prompts), 1, 1, 1, 1, MAX_NUM_WORDS)
        self.token_sets = []
        for i, (prompt, words_) in enumerate(zip(prompts, words)):
            if type(words_) is str:
                words_ = [words_]
            s = set()
            for word in words_:
                ind = ptp_utils.get_word_inds(prompt, word, tokenizer)
                alpha_layers[i, :, :, :, :, ind] = 1
                s |= set(int(t) for t in ind)
            self.token_sets.append(sorted(s))
        self.alpha_layers = alpha_layers
        self.threshold = threshold

    def __call__(self, x_t, attention_store):
        maps = attention_store["down_cross"][2:4] + attention_store["up_cross"][:3]
        if len(self.token_sets) != 2 or x_t.shape[0] != 2 or any(m.shape[0] != 2 for m in maps):
            raise ValueError(f"LocalBlend: exactly two prompts (the reference's mask[:1] + mask[1:] against x_t broadcasts for two samples only and "
                             f"raises with more), got {len(self.token_sets)} prompts and x_t of shape {tuple(x_t.shape)}")
        if not maps or any(m.shape[1] != 16 * 16 for m in maps):
            raise ValueError("LocalBlend: needs the 16 x 16 cross-attention maps down_cross[2:4] + up_cross[:3] in the store")
        x = x_t.float().contiguous()
        return ops.p2p_local_blend(maps, 16, maps[0].shape[2], self.token_sets, self.threshold, x).to(x_t.dtype)


class AttentionControl(abc.ABC):
    """:88-124.  Called by the registration's adapter as controller(attn_module, is_cross, place_in_unet, B, N, core, **operands); every
    CrossAttention call counts, and the step ends after num_att_layers of them."""

    def step_callback(self, x_t):
        return x_t

    def between_steps(self):
        return

    @property
    def num_uncond_att_layers(self):
        return 0        # LOW_RESOURCE is not built

    @abc.abstractmethod
    def forward(self, attn, is_cross, place_in_unet, B, N, core, **operands):
        raise NotImplementedError

    def __call__(self, attn, is_cross, place_in_unet, B, N, core, **operands):
        out = self.forward(attn, is_cross, place_in_unet, B, N, core, **operands)
        self.cur_att_layer += 1
        if self.cur_att_layer == self.num_att_layers + self.num_uncond_att_layers:
            self.cur_att_layer = 0
            self.cur_step += 1
            self.between_steps()
        return out

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0

    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0


class EmptyControl(AttentionControl):
    """:126-129"""

    def forward(self, attn, is_cross, place_in_unet, B, N, core, **operands):
        return core()


def _halves(B):
    if B % 2 or B < 2:
        raise ValueError(f"prompt2prompt: the batch is [unconditional half, conditional half], got {B} samples")
    return B // 2


class AttentionStore(AttentionControl):
    """:132-164.  attention_store[key][i]: fp32 [P, N, Nk], the head sum of call i of that place, summed over the steps so far; store_heads[key][i]:
    its head count.  Only cross-attention calls are stored (module docstring)."""

    @staticmethod
    def get_empty_store():
        return {"down_cross": [], "mid_cross": [], "up_cross": [], "down_self": [], "mid_self": [], "up_self": []}

    def _entry(self, place, P, N, Nk, heads, device):
        """(buffer, accumulate) of this call: created at its first visit, added to afterwards"""
        key = f"{place}_cross"
        i = self._pos[key]
        self._pos[key] = i + 1
        bufs = self.attention_store[key]
        if i == len(bufs):
            bufs.append(torch.empty(P, N, Nk, dtype=torch.float32, device=device))
            self.store_heads[key].append(heads)
            return bufs[i], False
        if tuple(bufs[i].shape) != (P, N, Nk):
            raise ValueError(f"AttentionStore: call {i} of {key} had shape {tuple(bufs[i].shape)} and now has {(P, N, Nk)}; reset() between runs")
        return bufs[i], True

    def _store_only(self, attn, place, B, N, q, kv, Nk):
        P = _halves(B)
        h, d = attn.heads, attn.dim_head
        inner = h * d
        buf, acc = self._entry(place, P, N, Nk, h, q.device)
        ops.attention_p2p(q[P * N:], kv[P * Nk:], None, P, h, N, Nk, d, attn.scale, (N * inner, d, inner), (Nk * 2 * inner, d, 2 * inner), (0, 0, 0),
                          list(range(P)), store=buf, store_row=list(range(P)), accumulate=acc, want_out=False)

    def forward(self, attn, is_cross, place_in_unet, B, N, core, **operands):
        if is_cross and N <= 32 ** 2:                      # :134: avoid memory overhead
            self._store_only(attn, place_in_unet, B, N, operands["q"], operands["kv"], operands["Nk"])
        return core()

    def between_steps(self):
        self._pos = {k: 0 for k in self.attention_store}

    def get_average_attention(self):
        """:147-149 per stored call: the mean over heads and steps, fp32 [P, N, Nk] (the reference keeps the heads apart: [P h, N, Nk])"""
        return {key: [b / (self.store_heads[key][i] * self.cur_step) for i, b in enumerate(bufs)] for key, bufs in self.attention_store.items()}

    def reset(self):
        super().reset()
        self.attention_store = self.get_empty_store()
        self.store_heads = self.get_empty_store()
        self._pos = {k: 0 for k in self.attention_store}

    def __init__(self):
        super().__init__()
        self.attention_store = self.get_empty_store()
        self.store_heads = self.get_empty_store()
        self._pos = {k: 0 for k in self.attention_store}


class AttentionControlEdit(AttentionStore, abc.ABC):
    """:167-210"""

    def step_callback(self, x_t):
        if self.local_blend is not None:
            x_t = self.local_blend(x_t, self.attention_store)
        return x_t

    @abc.abstractmethod
    def edit_tables(self):
        """(M [P-1, 77, 77] or None = identity, c0 [P-1, 77], d0 [P-1, 77]) of replace_cross_attention(base, own) = (base M) c0 + own d0, host fp32"""
        raise NotImplementedError

    def step_tables(self):
        """(M, c, d) of the current step: c = c0 a, d = d0 a + 1 - a with a = cross_replace_alpha[cur_step] (:192-193)"""
        a = self.cross_replace_alpha[self.cur_step].reshape(self.batch_size - 1, MAX_NUM_WORDS)
        M, c0, d0 = self.edit_tables()
        return M, c0 * a, d0 * a + 1 - a

    def _device_tables(self, device):
        key = (self.cur_step, str(device))
        if self._dev.get("key") != key:
            P = self.batch_size
            M, c, d = self.step_tables()
            live = bool((c != 0).any()) or bool((d != 1).any())
            cd = torch.zeros(2, P, MAX_NUM_WORDS)
            cd[0, 1:], cd[1, 1:] = c, d
            cd = cd.to(device)
            if "M" not in self._dev or self._dev["M_dev"] != str(device):
                Mf = None
                if M is not None:
                    Mf = torch.zeros(P, MAX_NUM_WORDS, MAX_NUM_WORDS)
                    Mf[1:] = M
                    Mf = Mf.to(device)
                self._dev["M"], self._dev["M_dev"] = Mf, str(device)
            self._dev.update(key=key, live=live, c=cd[0], d=cd[1])
        return self._dev["live"], self._dev["M"], self._dev["c"], self._dev["d"]

    def _edited_cross(self, attn, place, B, N, q, kv, Nk, M, c, d):
        P = _halves(B)
        h, dh = attn.heads, attn.dim_head
        inner = h * dh
        qs, ks = (N * inner, dh, inner), (Nk * 2 * inner, dh, 2 * inner)
        out = torch.empty(B, N, inner, dtype=q.dtype, device=q.device)
        buf, acc, rows = None, False, None
        if N <= 32 ** 2:
            buf, acc = self._entry(place, P, N, Nk, h, q.device)
            rows = list(range(P))
        kv2 = kv[P * Nk:]
        ops.attention_p2p(q[P * N:], kv2, kv2[:, inner:], P, h, N, Nk, dh, attn.scale, qs, ks, ks, [0] * P, M=M, c=c, d=d, store=buf, store_row=rows,
                          accumulate=acc, out=out[P:])
        # then the unconditional half AND the base through the plain launch (same stream: it overwrites the base's rows), so that prompt 0 keeps
        # the bits of a run without a controller
        ops.attention(q, kv, kv[:, inner:], P + 1, h, N, Nk, dh, attn.scale, qs, ks, ks, out=out[:P + 1])
        return out

    def _replaced_self(self, attn, B, N, qkv):
        P = _halves(B)
        h, d = attn.heads, attn.dim_head
        inner = h * d
        s, s0 = (N * 3 * inner, d, 3 * inner), (0, d, 3 * inner)
        out = torch.empty(B, N, inner, dtype=qkv.dtype, device=qkv.device)
        ops.attention(qkv, qkv[:, inner:], qkv[:, 2 * inner:], P + 1, h, N, N, d, attn.scale, s, s, s, out=out[:P + 1])
        base, own = qkv[P * N:], qkv[(P + 1) * N:]
        ops.attention(base, base[:, inner:], own[:, 2 * inner:], P - 1, h, N, N, d, attn.scale, s0, s0, s, out=out[P + 1:])
        return out

    def forward(self, attn, is_cross, place_in_unet, B, N, core, **operands):
        if _halves(B) != self.batch_size:
            raise ValueError(f"{type(self).__name__}: built for {self.batch_size} prompts, got a batch of {B} samples")
        if is_cross:
            q, kv, Nk = operands["q"], operands["kv"], operands["Nk"]
            if Nk != MAX_NUM_WORDS:
                raise ValueError(f"{type(self).__name__}: the tables hold {MAX_NUM_WORDS} tokens, the context has {Nk}")
            live, M, c, d = self._device_tables(q.device)
            if not live:
                return super().forward(attn, is_cross, place_in_unet, B, N, core, **operands)
            self.controlled.append((self.cur_step, self.cur_att_layer, "cross"))
            return self._edited_cross(attn, place_in_unet, B, N, q, kv, Nk, M, c, d)
        if self.num_self_replace[0] <= self.cur_step < self.num_self_replace[1] and N <= 16 ** 2 and self.batch_size > 1:
            self.controlled.append((self.cur_step, self.cur_att_layer, "self"))
            return self._replaced_self(attn, B, N, operands["qkv"])
        return core()

    def reset(self):
        super().reset()
        self.controlled = []
        self._dev = {}

    def __init__(self, prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend, tokenizer=None):
        super().__init__()
        tokenizer = _need(tokenizer, type(self).__name__)
        self.batch_size = len(prompts)
        self.cross_replace_alpha = ptp_utils.get_time_words_attention_alpha(prompts, num_steps, cross_replace_steps, tokenizer)
        if type(self_replace_steps) is float:
            self_replace_steps = 0, self_replace_steps
        self.num_self_replace = int(num_steps * self_replace_steps[0]), int(num_steps * self_replace_steps[1])
        self.local_blend = local_blend
        self.controlled = []   # (cur_step, cur_att_layer, "cross" | "self") of the calls this controller took over, in order
        self._dev = {}


class AttentionReplace(AttentionControlEdit):
    """:212-221"""

    def edit_tables(self):
        n = self.batch_size - 1
        return self.mapper, torch.ones(n, MAX_NUM_WORDS), torch.zeros(n, MAX_NUM_WORDS)

    def __init__(self, prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend=None, tokenizer=None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend, tokenizer=tokenizer)
        self.mapper = seq_aligner.get_replacement_mapper(prompts, tokenizer)


class AttentionRefine(AttentionControlEdit):
    """:224-237.  The gather attn_base[:, :, mapper] is the one-hot M[i, j] = (i == mapper[j]); index -1 is Python's last token, where alphas is 0."""

    def edit_tables(self):
        n = self.batch_size - 1
        M = torch.zeros(n, MAX_NUM_WORDS, MAX_NUM_WORDS)
        cols = torch.arange(MAX_NUM_WORDS)
        for e in range(n):
            M[e, self.mapper[e] % MAX_NUM_WORDS, cols] = 1.0
        al = self.alphas.reshape(n, MAX_NUM_WORDS)
        return M, al, 1 - al

    def __init__(self, prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend=None, tokenizer=None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend, tokenizer=tokenizer)
        self.mapper, alphas = seq_aligner.get_refinement_mapper(prompts, tokenizer)
        self.alphas = alphas.reshape(alphas.shape[0], 1, 1, alphas.shape[1])


class AttentionReweight(AttentionControlEdit):
    """:240-253"""

    def edit_tables(self):
        n = self.batch_size - 1
        eq = self.equalizer.reshape(-1, MAX_NUM_WORDS).expand(n, -1)
        if self.prev_controller is not None:
            M, c0, d0 = self.prev_controller.edit_tables()
            return M, c0 * eq, d0 * eq
        return None, eq.clone(), torch.zeros(n, MAX_NUM_WORDS)

    def __init__(self, prompts, num_steps, cross_replace_steps, self_replace_steps, equalizer, local_blend=None, controller=None, tokenizer=None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend, tokenizer=tokenizer)
        self.equalizer = equalizer.float()
        self.prev_controller = controller


def get_equalizer(text, word_select, values, tokenizer=None):
    """:256-265: fp32 [len(values), 77], `values` at the tokens of the selected word(s) and 1 elsewhere"""
    tokenizer = _need(tokenizer, "get_equalizer")
    if type(word_select) is int or type(word_select) is str:
        word_select = (word_select,)
    equalizer = torch.ones(len(values), MAX_NUM_WORDS)
    values = torch.tensor(values, dtype=torch.float32)
    for word in word_select:
        inds = ptp_utils.get_word_inds(text, word, tokenizer)
        equalizer[:, inds] = values
    return equalizer


def aggregate_attention(attention_store, res, from_where, is_cross, select, prompts):
    """:270-281: the reference concatenates the per-head maps of every stored call with res^2 queries and takes sum / count; that is
    (sum of head sums) / (sum of head counts), whether or not the calls have equal head counts.  fp32 [res, res, Nk] on the CPU."""
    if not is_cross:
        raise ValueError("aggregate_attention: self-attention maps are not stored (their only reader is a visualisation)")
    total, heads = None, 0
    for location in from_where:
        key = f"{location}_cross"
        for buf, h in zip(attention_store.attention_store[key], attention_store.store_heads[key]):
            if buf.shape[1] == res ** 2:
                if buf.shape[0] != len(prompts):
                    raise ValueError(f"aggregate_attention: the store holds {buf.shape[0]} prompts, got {len(prompts)}")
                m = buf[select].float() / attention_store.cur_step
                total = m if total is None else total + m
                heads += h
    if total is None:
        raise ValueError(f"aggregate_attention: no stored cross-attention map with {res} x {res} queries in {tuple(from_where)}")
    return (total / heads).reshape(res, res, -1).cpu()


def mask_from_CA(attention_store, res, from_where, prompts, key_words, select=0, tokenizer=None):
    """:319-343, the reference's host path: per token, 255 map / max truncated to uint8, PIL resize to 256 x 256, > 0.85 mean; the union over the key
    words' positions.  Kept quirk: a word's index in prompt.split() plus 1 is used as its token index.  Returns a PIL image of 0 / 255."""
    from PIL import Image
    tokenizer = _need(tokenizer, "mask_from_CA")
    words = prompts[select].split()
    positions = [words.index(w) + 1 if w in words else -1 for w in key_words]
    tokens = tokenizer.encode(prompts[select])
    maps = aggregate_attention(attention_store, res, from_where, True, select, prompts=prompts)
    mask_sum = 0
    for i in range(1, len(tokens)):
        if i not in positions:
            continue
        image = maps[:, :, i]
        image = 255 * image / image.max()
        image = image.unsqueeze(-1).expand(*image.shape, 3)
        image = image.numpy().astype(np.uint8)
        image = np.array(Image.fromarray(image).resize((256, 256)))
        mask_sum = mask_sum + np.where(image > np.mean(image) * 0.85, 1, 0)
    mask = np.where(mask_sum > 0, 1, 0) * 255
    if np.ndim(mask) == 0:
        mask = np.zeros((256, 256, 3), dtype=np.int64)
    return Image.fromarray(mask.astype(np.uint8))
