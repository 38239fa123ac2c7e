"""Mirror of AnyEdit_Collection/other_modules/masactrl/masactrl.py (reference file:line cited per class) on the HIP attention operators.

Names and constructor signatures are the reference's.  The batch is the reference's [u_s, u_t, c_s, c_t] (unconditional half, conditional half;
source first in each half: DDIMSampler's `[uncond, cond]` order, ddim.py:156-171).  A controlled self-attention never forms sim or attn:
  * plain control is a choice of strides on the existing `ops.attention` (no new kernel);
  * the mask-guided variants are ONE `ops.attention_mutual` launch for all four branches: sample b reads K / V of its half's source, a target
    query is allowed the source keys of its own class (the reference's foreground / background softmaxes blended by a 0 / 1 mask select one
    of the two per query), source rows take every key;
  * the automatic variant sums the 16x16 cross-attention maps with `ops.attention_token_map` and turns them into classes with
    `ops.masactrl_classes`, without a host synchronisation.
Not built: MutualSelfAttentionControlUnion (masactrl.py:75-111), SDXL layer counts beyond the table, mask_save_dir images, non-binary masks."""
import torch
import torch.nn.functional as F

from anyedit_amd import ops
from .masactrl_utils import AttentionBase


def _side(N):
    s = int(round(N ** 0.5))
    if s * s != N:
        raise ValueError(f"MasaCtrl: a masked self-attention needs a square token grid, got {N} tokens")
    return s


class MutualSelfAttentionControl(AttentionBase):
    """masactrl.py:14-72.  From `start_step` / `start_layer` on, every self-attention of a half reads the keys and values of the half's first
    sample.  No new kernel: a stride-only call of `ops.attention` as a batch of 2 halves with n N query rows each and a K / V batch stride of
    n N 3 inner, i.e. "sample b reads K / V of sample (b // n) n"."""
    MODEL_TYPE = {"SD": 16, "SDXL": 70}

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, model_type="SD"):
        super().__init__()
        self.total_steps = total_steps
        self.total_layers = self.MODEL_TYPE.get(model_type, 16)
        self.start_step = start_step
        self.start_layer = start_layer
        self.layer_idx = layer_idx if layer_idx is not None else list(range(start_layer, self.total_layers))
        self.step_idx = step_idx if step_idx is not None else list(range(start_step, total_steps))
        self.controlled = []   # (cur_step, cur_att_layer) of the calls this editor took over, in order

    def reset(self):
        super().reset()
        self.controlled = []

    def _is_controlled(self, is_cross):
        return not (is_cross or self.cur_step not in self.step_idx or self.cur_att_layer // 2 not in self.layer_idx)   # masactrl.py:60

    def _plain(self, attn, B, N, qkv):
        if B % 2:
            raise ValueError(f"MasaCtrl: the batch is [unconditional half, conditional half], got {B} samples")
        h, d = attn.heads, attn.dim_head
        inner = h * d
        n = B // 2
        qs = (n * N * 3 * inner, d, 3 * inner)
        o = ops.attention(qkv, qkv[:, inner:], qkv[:, 2 * inner:], 2, h, n * N, N, d, attn.scale, qs, qs, qs)
        return o.reshape(B, N, inner)

    def forward(self, attn, is_cross, B, N, core, **operands):
        if not self._is_controlled(is_cross):
            return super().forward(attn, is_cross, B, N, core, **operands)
        self.controlled.append((self.cur_step, self.cur_att_layer))
        return self._plain(attn, B, N, operands["qkv"])


def _mutual(attn, B, N, qkv, src, qcls, kcls, kcnt):
    h, d = attn.heads, attn.dim_head
    inner = h * d
    s = (N * 3 * inner, d, 3 * inner)
    return ops.attention_mutual(qkv, qkv[:, inner:], qkv[:, 2 * inner:], B, h, N, d, attn.scale, s, s, s, src, qcls=qcls, kcls=kcls, kcnt=kcnt)


class MutualSelfAttentionControlMask(MutualSelfAttentionControl):
    """masactrl.py:114-193.  mask_s / mask_t: (h, w) tensors of 0 and 1 (checked once, on the host, here), both or neither; exactly two samples
    per half.  The classes of a resolution come from F.interpolate at its first use."""

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, mask_s=None, mask_t=None, mask_save_dir=None,
                 model_type="SD"):
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps, model_type)
        if (mask_s is None) != (mask_t is None):
            raise ValueError("MutualSelfAttentionControlMask: give mask_s and mask_t, or neither")
        if mask_save_dir is not None:
            raise ValueError("MutualSelfAttentionControlMask: mask_save_dir is not supported")
        for name, m in (("mask_s", mask_s), ("mask_t", mask_t)):
            if m is None:
                continue
            if not torch.is_tensor(m) or m.dim() != 2:
                raise ValueError(f"MutualSelfAttentionControlMask: {name} must be an (h, w) tensor")
            mc = m.detach().float().cpu()
            if not bool(((mc == 0) | (mc == 1)).all()):
                raise ValueError(f"MutualSelfAttentionControlMask: {name} must hold only 0 and 1")
        self.mask_s = None if mask_s is None else mask_s.detach().float().cpu()
        self.mask_t = None if mask_t is None else mask_t.detach().float().cpu()
        self._cls = {}

    def classes(self, N, device):
        """(qcls [4, N], kcls [4, N], kcnt [4, 2]) of the [u_s, u_t, c_s, c_t] batch at N tokens"""
        key = (N, str(device))
        if key not in self._cls:
            s = _side(N)
            ks = F.interpolate(self.mask_s[None, None], (s, s)).flatten().to(torch.uint8)   # masactrl.py:148-149
            qt = F.interpolate(self.mask_t[None, None], (s, s)).flatten().to(torch.uint8)   # masactrl.py:187-188
            qcls = torch.full((4, N), ops.CLS_ANY, dtype=torch.uint8)
            qcls[1] = qt
            qcls[3] = qt
            kcls = ks[None].repeat(4, 1)
            ones = int(ks.sum())
            kcnt = torch.tensor([[N - ones, ones]] * 4, dtype=torch.int32)
            self._cls[key] = tuple(t.contiguous().to(device) for t in (qcls, kcls, kcnt))
        return self._cls[key]

    def forward(self, attn, is_cross, B, N, core, **operands):
        if not self._is_controlled(is_cross):
            return AttentionBase.forward(self, attn, is_cross, B, N, core, **operands)
        if B != 4:
            raise ValueError(f"MutualSelfAttentionControlMask: exactly two samples per half ([u_s, u_t, c_s, c_t]), got a batch of {B}")
        self.controlled.append((self.cur_step, self.cur_att_layer))
        qkv = operands["qkv"]
        if self.mask_s is None:
            return self._plain(attn, B, N, qkv)
        qcls, kcls, kcnt = self.classes(N, qkv.device)
        return _mutual(attn, B, N, qkv, (0, 0, 2, 2), qcls, kcls, kcnt)


class MutualSelfAttentionControlMaskAuto(MutualSelfAttentionControl):
    """masactrl.py:196-334.  Cross-attention calls with 256 queries add their head-averaged probability map (summed over the sample's token set)
    to the step's buffer; a controlled self-attention takes the source classes from sample -2 / ref_token_idx and the query classes from sample
    -1 / cur_token_idx, and is plain mutual attention while no map has been collected in this step.  (The reference's mean over the collected
    maps is a positive factor its min-max normalisation removes: the buffer holds their sum.)"""

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, thres=0.1, ref_token_idx=[1], cur_token_idx=[1],
                 mask_save_dir=None, model_type="SD"):
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps, model_type)
        if mask_save_dir is not None:
            raise ValueError("MutualSelfAttentionControlMaskAuto: mask_save_dir is not supported")
        self.thres = thres
        self.ref_token_idx = [ref_token_idx] if isinstance(ref_token_idx, int) else list(ref_token_idx)
        self.cur_token_idx = [cur_token_idx] if isinstance(cur_token_idx, int) else list(cur_token_idx)
        self.n_maps = 0        # 16x16 cross-attention maps collected in this step (len(self.cross_attns) of the reference)
        self._map = None       # fp32 [B, 256]: their sum
        self._cls = {}         # (step, N, n_maps) -> (cls [2B, N], counts [2B, 2])

    def after_step(self):
        self.n_maps = 0
        self._cls = {}

    def reset(self):
        super().reset()
        self.after_step()

    def classes(self, B, N, device):
        key = (self.cur_step, N, self.n_maps)
        if key not in self._cls:
            cls = torch.empty(2 * B, N, dtype=torch.uint8, device=device)
            cls[B:].fill_(ops.CLS_ANY)                 # rows B .. 2B-1: query classes; the source rows stay "any"
            counts = torch.zeros(2 * B, 2, dtype=torch.int32, device=device)
            pairs = [(B - 2, 0), (B - 2, 2), (B - 1, B + 1), (B - 1, B + 3)]
            ops.masactrl_classes(self._map, 16, _side(N), self.thres, pairs, cls, counts)
            self._cls = {k: v for k, v in self._cls.items() if k[0] == self.cur_step}
            self._cls[key] = (cls, counts)
        return self._cls[key]

    def forward(self, attn, is_cross, B, N, core, **operands):
        if is_cross and N == 16 * 16:                  # masactrl.py:277-280
            h, d = attn.heads, attn.dim_head
            inner = h * d
            q, kv, Nk = operands["q"], operands["kv"], operands["Nk"]
            if self._map is None or self._map.shape[0] != B or self._map.device != q.device:
                self._map = torch.empty(B, N, dtype=torch.float32, device=q.device)
            sets = [self.ref_token_idx] * (B - 1) + [self.cur_token_idx]
            ops.attention_token_map(q, kv, B, h, N, Nk, d, attn.scale, (N * inner, d, inner), (Nk * 2 * inner, d, 2 * inner), sets, out=self._map,
                                    accumulate=self.n_maps > 0)
            self.n_maps += 1
        if not self._is_controlled(is_cross):
            return AttentionBase.forward(self, attn, is_cross, B, N, core, **operands)
        if B != 4:
            raise ValueError(f"MutualSelfAttentionControlMaskAuto: exactly two samples per half ([u_s, u_t, c_s, c_t]), got a batch of {B}")
        self.controlled.append((self.cur_step, self.cur_att_layer))
        qkv = operands["qkv"]
        if self.n_maps == 0:                           # masactrl.py:295-298
            return self._plain(attn, B, N, qkv)
        cls, counts = self.classes(B, N, qkv.device)
        return _mutual(attn, B, N, qkv, (0, 0, 2, 2), cls[B:], cls[:B], counts[:B])
