"""float64 statements of the MasaCtrl formulas (csrc/masactrl.hip, anyedit_amd/masactrl), written from the definitions:

  mutual attention   out[b, h, i] = sum_j p_ij v[s, h, j],  s = src[b],  p_i = softmax_j over the ALLOWED keys of scale q[b, h, i] . k[s, h, j];
                     key j is allowed for query (b, i) iff qcls is None or qcls[b, i] == 255 or kcls[s, j] == qcls[b, i]; a query with no allowed
                     key takes the plain mean of v[s, h, :] (every logit equal).
  token map          out[b, i] = 1/H sum_h sum_{j in set_b} softmax_j(scale q[b, h, i] . k[b, h, j]).
  classes            x S x S -> (x - min) / (max - min) -> nearest resize to R x R, source index min(floor(dst * S / R), S - 1) with the product in
                     fp32 (F.interpolate's rule) -> 1 where >= thres; a constant map gives zeros.

`cpu_ops(...)` dresses them as the operators of `anyedit_amd.ops` that the editors call (same argument lists, operands addressed through the same
element strides), so the editor classes can be driven on the CPU."""
import numpy as np
import torch

F64 = torch.float64
CLS_ANY = 255


def allowed_keys(qc, kc):
    """bool [N, Nk]: which keys each query may read.  qc: int [N] or None; kc: int [Nk] or None."""
    if qc is None:
        return None
    qc, kc = torch.as_tensor(qc).long(), torch.as_tensor(kc).long()
    return (qc[:, None] == CLS_ANY) | (qc[:, None] == kc[None, :])


def mutual_ref(Q, K, V, scale, src, qcls=None, kcls=None):
    """Q, K, V: float64 [B, H, N, D].  Returns (r, sv): softmax(S) V and softmax(S) |V|, both [B, H, N, D]."""
    B, H, N, D = Q.shape
    r, sv = torch.empty_like(Q), torch.empty_like(Q)
    for b in range(B):
        s = int(src[b])
        S = torch.einsum("hid,hjd->hij", Q[b], K[s]) * scale
        al = allowed_keys(None if qcls is None else qcls[b], None if qcls is None else kcls[s])
        if al is not None:
            empty = ~al.any(1)
            S = S.masked_fill(~al[None], float("-inf"))
            S[:, empty, :] = 0.0                       # no key of the class: all logits equal
        P = torch.softmax(S, -1)
        r[b] = P @ V[s]
        sv[b] = P @ V[s].abs()
    return r, sv


def token_map_ref(Q, K, scale, sets):
    """Q [B, H, N, D], K [B, H, Nk, D] float64; sets: B iterables of key indices.  Returns (map [B, N], qk_abs [B, N]): the map and
    max_{h, j} scale sum_d |q_d| |k_jd| per query (what a per-logit error bound scales with)."""
    B, H, N, D = Q.shape
    out = torch.zeros(B, N, dtype=F64)
    P = torch.softmax(torch.einsum("bhid,bhjd->bhij", Q, K) * scale, -1)
    for b in range(B):
        idx = torch.tensor(sorted(set(int(t) for t in sets[b])), dtype=torch.long)
        out[b] = P[b][:, :, idx].sum(-1).mean(0) if len(idx) else 0.0
    qk_abs = (torch.einsum("bhid,bhjd->bhij", Q.abs(), K.abs()) * scale).amax((1, 3))
    return out, qk_abs


def nearest_index(R, S):
    """F.interpolate(mode='nearest') source indices of R outputs over S inputs: min(floor(dst * (S / R)), S - 1), scale and product in fp32"""
    sc = np.float32(S) / np.float32(R)
    return np.minimum(np.floor(np.arange(R, dtype=np.float32) * sc).astype(np.int64), S - 1)


def classes_ref(x, S, R, thres):
    """x: [S*S] values.  Returns (cls uint8 [R*R], counts [2], norm float64 [R*R]: the normalised value each output pixel compares with thres)."""
    x = torch.as_tensor(x).to(F64).reshape(S, S)
    mn, mx = x.min(), x.max()
    idx = torch.from_numpy(nearest_index(R, S))
    if mx > mn:
        norm = ((x - mn) / (mx - mn))[idx][:, idx].reshape(-1)
        cls = (norm >= thres).to(torch.uint8)
    else:
        norm = torch.full((R * R,), float("nan"), dtype=F64)
        cls = torch.zeros(R * R, dtype=torch.uint8)
    ones = int(cls.sum())
    return cls, torch.tensor([R * R - ones, ones], dtype=torch.int32), norm


# ------------------------------------------------------------------------------------------- the operators the editors call, on the CPU
def view4(t, B, H, n, D, st):
    return t.as_strided((B, H, n, D), tuple(st) + (1,), t.storage_offset()).to(F64)


class cpu_ops:
    """Stand-ins for ops.attention / attention_mutual / attention_token_map / masactrl_classes with the same argument lists, computing the float64
    statements above on CPU tensors of any float dtype.  `calls` records (name, key facts) of every launch the editor asked for."""

    def __init__(self):
        self.calls = []

    def attention(self, q, k, v, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, key_mask=None, **kw):
        assert not kw and key_mask is None
        self.calls.append(("attention", B, Nq, Nk))
        Q, K, V = view4(q, B, H, Nq, D, q_strides), view4(k, B, H, Nk, D, k_strides), view4(v, B, H, Nk, D, v_strides)
        P = torch.softmax(torch.einsum("bhid,bhjd->bhij", Q, K) * scale, -1)
        return (P @ V).permute(0, 2, 1, 3).reshape(B, Nq, H * D)

    def attention_mutual(self, q, k, v, B, H, N, D, scale, q_strides, k_strides, v_strides, src, qcls=None, kcls=None, kcnt=None, **kw):
        assert not kw
        self.calls.append(("attention_mutual", B, N, tuple(src)))
        Q, K, V = view4(q, B, H, N, D, q_strides), view4(k, B, H, N, D, k_strides), view4(v, B, H, N, D, v_strides)
        if qcls is not None:
            for b in range(B):   # the counts the kernel trusts must describe kcls
                s = int(src[b])
                assert int(kcnt[s, 1]) == int((kcls[s] == 1).sum()) and int(kcnt[s, 0]) == int((kcls[s] == 0).sum())
        r, _ = mutual_ref(Q, K, V, scale, src, qcls, kcls)
        return r.permute(0, 2, 1, 3).reshape(B, N, H * D)

    def attention_token_map(self, q, k, B, H, N, Nk, D, scale, q_strides, k_strides, token_sets, out=None, accumulate=False):
        self.calls.append(("attention_token_map", B, N, Nk, bool(accumulate)))
        m, _ = token_map_ref(view4(q, B, H, N, D, q_strides), view4(k, B, H, Nk, D, k_strides), scale, token_sets)
        if out is None:
            out = torch.zeros(B, N, dtype=torch.float64)
        if accumulate:
            out += m.to(out.dtype)
        else:
            out.copy_(m)
        return out

    def masactrl_classes(self, maps, S, R, thres, pairs, cls, counts):
        self.calls.append(("masactrl_classes", S, R, tuple(pairs)))
        for s, o in pairs:
            c, n, _ = classes_ref(maps[s], S, R, thres)
            cls[o] = c
            counts[o] = n
        return cls, counts

    def install(self, monkeypatch, ops):
        for name in ("attention", "attention_mutual", "attention_token_map", "masactrl_classes"):
            monkeypatch.setattr(ops, name, getattr(self, name))


# ------------------------------------------------------------------------------------------- the golden's protocol (tools/gen_golden_masactrl.py)
def call_inputs(g, step, layer):
    """q, k, v ([B h, n, d] fp32, the reference hook's layout) of attention call `layer` of denoising step `step`: the stored base operands, the
    queries scaled by a factor that differs from call to call (so that no two calls share an output)."""
    is_cross = layer % 2 == 1
    f = 1.0 + 0.125 * ((3 * step + layer) % 5)
    if is_cross:
        return True, g["q_cross"] * f, g["k_cross"], g["v_cross"]
    return False, g["q_self"] * f, g["k_self"], g["v_self"]


def bf16_bits_to_f32(a):
    if a.dtype != np.uint16:
        return torch.from_numpy(a)
    return torch.from_numpy((np.ascontiguousarray(a).astype(np.uint32) << 16).view(np.float32))


def load_golden(path):
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    for k in ("q_self", "k_self", "v_self", "q_cross", "k_cross", "v_cross"):
        g[k] = bf16_bits_to_f32(g[k])
    return g


# protocol constants of the golden
G_H, G_D, G_N, G_NK, G_B = 2, 8, 256, 8, 4
G_LAYERS, G_STEPS, G_START_STEP, G_START_LAYER = 6, 2, 1, 1
G_ROWS = (0, 1, 15, 16, 17, 31, 32, 63, 64, 100, 127, 128, 129, 136, 137, 152, 153, 200, 239, 240, 254, 255)
G_AUTO = dict(thres=0.5, ref_token_idx=[1], cur_token_idx=[1, 2])
G_CONFIGS = ("base", "plain", "mask", "mask_empty", "mask_one", "auto")


def golden_masks(name):
    """(mask_s, mask_t) of a mask-guided configuration: `mask` a blob and a shifted blob at 32 x 32 (resized down by the editors), `mask_empty` a
    source mask without any foreground (the foreground class is empty), `mask_one` a source mask with a single foreground key at 16 x 16."""
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    blob = (((yy - 14) ** 2 + (xx - 12) ** 2) < 81).float()
    blob_t = (((yy - 18) ** 2 + (xx - 20) ** 2) < 64).float()
    if name == "mask":
        return blob, blob_t
    if name == "mask_empty":
        return torch.zeros(32, 32), blob_t
    if name == "mask_one":
        one = torch.zeros(16, 16)
        one[9, 8] = 1.0
        return one, blob_t[::2, ::2].contiguous()
    raise KeyError(name)


# ------------------------------------------------------------------------------------------- cases of the classes kernel (CPU and GPU suites share them)
CLS_BOUND = 2.0 ** -22   # |fp32 (x - min) / (max - min) - float64| for values in [0, 1]: two subtractions and one division, each within 2^-24
                         # relative of a value <= 1, plus the threshold's own rounding to fp32 (2^-25): 3.5 * 2^-24 < 2^-22
CLASS_CASES = [  # (id, S, R, thres, kind, seed)
    ("4to4", 4, 4, 0.5, "random", 1), ("4to8", 4, 8, 0.3, "random", 2), ("16to16", 16, 16, 0.1, "random", 3), ("16to32", 16, 32, 0.5, "random", 4),
    ("16to64", 16, 64, 0.7, "random", 5), ("constant", 16, 32, 0.5, "constant", 6), ("exact", 4, 8, 0.5, "exact", 7),
]


def class_case_maps(S, kind, seed, nmaps=3):
    """fp32 [nmaps, S*S] maps of a case: positive, like sums of probabilities.  `constant`: map 1 is constant.  `exact`: map 1 holds 0, 0.5 and 1 among
    multiples of 1/8, so that its normalised values are exact in fp32 and float64 alike and 0.5 meets the threshold 0.5 exactly (class 1)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    maps = torch.rand(nmaps, S * S, generator=gen) * 3.0 + 0.01
    if kind == "constant":
        maps[1] = 0.625
    if kind == "exact":
        maps[1] = torch.randint(0, 9, (S * S,), generator=gen).float() / 8.0
        maps[1, 0], maps[1, 1], maps[1, 2] = 0.0, 0.5, 1.0
    return maps.float()
