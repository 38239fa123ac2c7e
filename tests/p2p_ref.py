"""float64 statements of the Prompt-to-Prompt formulas (csrc/prompt2prompt.hip, anyedit_amd/prompt2prompt), written from the definitions:

  edited attention   P_base = softmax_j(scale q_s k_s^T), P_own = softmax_j(scale q_b k_b^T), s = base[b];
                     P' = (P_base M_b) * c_b + P_own * d_b for s != b (M_b = I when M is None), P' = P_own for s == b; out_b = P' v_b;
                     store[store_row[b]] (+)= sum_h P'[b, h].
  local blend        m_b = sum_layers sum_{j in set_b} map_l[b, :, j] -> 3x3 max-pool (stride 1, pad 1) -> nearest resize S -> (h, w), source index
                     min(floor(dst * S / out), S - 1) with the product in fp32 (F.interpolate's rule) -> / its maximum -> > threshold ->
                     mask_0 or mask_1 -> out[1] = x[1] where the mask is set, else x[0]; out[0] = x[0].  A zero maximum gives an empty mask.

`cpu_ops` dresses them as the operators of `anyedit_amd.ops` that the controllers call, so the controller classes can be driven on the CPU.  The
toy tokenizer, the golden's protocol (tools/gen_golden_p2p.py) and the kernel cases and bounds that the CPU and GPU suites share follow."""
import math

import numpy as np
import torch

import masactrl_ref as MR

F64 = torch.float64
view4 = MR.view4
bf16_bits_to_f32 = MR.bf16_bits_to_f32


def p2p_ref(Q, K, V, scale, base, M=None, c=None, d=None):
    """Q [B, H, N, D], K / V [B, H, Nk, D] float64 (V may be None); M [B, Nk, Nk] or None, c / d [B, Nk].  Returns (out [B, H, N, D] or None,
    Pp [B, H, N, Nk] = P', W [B, H, N, Nk] = |c| (P_base |M|) + |d| P_own, the weights the rounding bound scales with; W = P_own if unedited)."""
    B = Q.shape[0]
    P = torch.softmax(torch.einsum("bhid,bhjd->bhij", Q, K) * scale, -1)
    Pp, W = P.clone(), P.clone()
    for b in range(B):
        s = int(base[b])
        if s == b:
            continue
        cb, db = c[b].to(F64), d[b].to(F64)
        if M is None:
            mix, amix = P[s], P[s]
        else:
            mix, amix = P[s] @ M[b].to(F64), P[s] @ M[b].to(F64).abs()
        Pp[b] = mix * cb + P[b] * db
        W[b] = amix * cb.abs() + P[b] * db.abs()
    out = None if V is None else Pp @ V
    return out, Pp, W


def qk_abs(Q, K, scale):
    """max over (b, h, i, j) of scale sum_d |q_d| |k_d|: what a per-logit fp32 error scales with"""
    return float((torch.einsum("bhid,bhjd->bhij", Q.abs(), K.abs()) * scale).max())


def eps_prob(D, Nk, qk):
    """Relative error of one fp32 probability of ae_attn_p2p_bf16, derived from its arithmetic (p2p_probs): a logit is an fp32 fma chain over D
    exact bf16 products, |ds| <= D 2^-24 sum_d |q_d| |k_d|; t = s c2 and t - m add 2^-23 |t|; v_exp_f32 is within 1 ulp (2^-23).  In natural
    units the logit error is E = (D + 2) 2^-24 qk, a probability e_j / sum e moves by at most 2 E (numerator and denominator) + 2^-23 (exp) + the
    wave sum of <= 128 non-negative terms in a 7-level tree (7 x 2^-24) + the division (2^-24): 2 E + 2^-20 with room."""
    return 2.0 * (D + 2) * 2.0 ** -24 * qk + 2.0 ** -20


def p2p_out_bound(ref, W, V, D, Nk, qk):
    """|got - ref| <= 2^-8 |ref| + kappa 2^-8 sum_j w_j |v_j|, the project's form.  kappa counts bf16 roundings on the probability path: the kernel
    has none (fp32 probabilities, fp32 P_base M, fp32 blend, fp32 fma over the keys), so kappa 2^-8 is replaced by the fp32 path's own relative
    error per term: eps_prob for each of the two softmaxes (already weighted by |c| |M| and |d| inside w), Nk 2^-24 for the fma chain over the base's
    tokens, 2 x 2^-24 for the blend, Nk 2^-24 for the fma chain over the keys: kappa 2^-8 := eps_prob + (2 Nk + 2) 2^-24.  The 2^-8 |ref| term is the
    one bf16 rounding of the output (half an ulp of 8 significand bits)."""
    k8 = eps_prob(D, Nk, qk) + (2 * Nk + 2) * 2.0 ** -24
    return 2.0 ** -8 * ref.abs() + k8 * (W @ V.abs()) + 1e-30


def p2p_store_bound(W, Nk, D, qk, H, launches=1):
    """Store: sum over heads of P' in fp32, no bf16 rounding anywhere: |got - ref| <= (eps_prob + (Nk + 2) 2^-24) sum_h w + (H + launches) 2^-24
    sum_h w for the head additions and the accumulate additions (each rounds a partial sum of magnitude <= sum_h w)."""
    k = eps_prob(D, Nk, qk) + (Nk + 2 + H + launches) * 2.0 ** -24
    return k * W.sum(1) + 1e-30


# ------------------------------------------------------------------------------------------- local blend
def nearest_index(R, S):
    return MR.nearest_index(R, S)


def blend_maps(maps, sets, S, h, w):
    """normalised maps, float64 [2, h, w] (NaN where the maximum is 0), from store maps [2, S S, Nk]"""
    out = torch.empty(2, h, w, dtype=F64)
    iy, ix = torch.from_numpy(nearest_index(h, S)), torch.from_numpy(nearest_index(w, S))
    for b in range(2):
        idx = torch.tensor(sorted(set(int(t) for t in sets[b])), dtype=torch.long)
        m = torch.zeros(S * S, dtype=F64)
        for mp in maps:
            m = m + mp[b].to(F64)[:, idx].sum(-1)
        m = torch.nn.functional.max_pool2d(m.reshape(1, 1, S, S), 3, 1, 1)[0, 0]
        r = m[iy][:, ix]
        mx = r.max()
        out[b] = r / mx if float(mx) != 0.0 else float("nan")
    return out


def blend_ref(maps, sets, S, thr, x):
    """(out, mask bool [h, w], norm [2, h, w]); thr is compared as the fp32 value the kernel receives"""
    h, w = x.shape[2:]
    norm = blend_maps(maps, sets, S, h, w)
    mask = (norm[0] > float(np.float32(thr))) | (norm[1] > float(np.float32(thr)))     # NaN compares false
    out = x.clone()
    out[1] = torch.where(mask[None], x[1], x[0])
    return out, mask, norm


def blend_band(nterms):
    """Width of the exclusion band around the threshold: the fp32 map value is a sequential sum of `nterms` non-negative terms (relative error
    <= nterms 2^-24), the maximum carries the same, the division adds 2^-24, the threshold's own rounding to fp32 2^-25 of a value <= 1: the
    normalised value (<= 1) moves by at most (2 nterms + 2) 2^-24."""
    return (2 * nterms + 2) * 2.0 ** -24


# ------------------------------------------------------------------------------------------- the operators the controllers call, on the CPU
class cpu_ops(MR.cpu_ops):
    """masactrl_ref.cpu_ops plus attention_p2p / p2p_local_blend; `attention` also honours `out=` (a [B, Nq, H D] buffer)"""

    def attention(self, q, k, v, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, out=None, **kw):
        r = super().attention(q, k, v, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, **kw)
        if out is not None:
            out.copy_(r.to(out.dtype))
            return out
        return r

    def attention_p2p(self, q, k, v, B, H, N, Nk, D, scale, q_strides, k_strides, v_strides, base, M=None, c=None, d=None, store=None, store_row=None,
                      accumulate=False, out=None, o_strides=None, want_out=True):
        self.calls.append(("attention_p2p", B, N, Nk, tuple(base), bool(want_out), None if store is None else bool(accumulate)))
        Q, K = view4(q, B, H, N, D, q_strides), view4(k, B, H, Nk, D, k_strides)
        V = view4(v, B, H, Nk, D, v_strides) if want_out else None
        r, Pp, _ = p2p_ref(Q, K, V, scale, base, M, c, d)
        if store is not None:
            for b in range(B):
                if store_row[b] >= 0:
                    s = Pp[b].sum(0).to(store.dtype)
                    store[store_row[b]] = store[store_row[b]] + s if accumulate else s
        if not want_out:
            return None
        r = r.permute(0, 2, 1, 3).reshape(B, N, H * D)
        if out is not None:
            out.copy_(r.to(out.dtype))
            return out
        return r

    def p2p_local_blend(self, maps, S, Nk, token_sets, threshold, x, out=None):
        self.calls.append(("p2p_local_blend", len(maps), S))
        if x.shape[0] != 2 or any(m.shape[0] != 2 for m in maps):
            raise ValueError("p2p_local_blend: exactly two samples")
        r, _, _ = blend_ref(maps, token_sets, S, threshold, x)
        if out is not None:
            out.copy_(r)
            return out
        return r

    def install(self, monkeypatch, ops):
        for name in ("attention", "attention_p2p", "p2p_local_blend"):
            monkeypatch.setattr(ops, name, getattr(self, name))


# ------------------------------------------------------------------------------------------- toy tokenizer
class ToyTokenizer:
    """Words of more than 5 letters become two pieces (w[:4], w[4:]); ids are handed out in order of first use.  encode() brackets the pieces
    with BOS = 0 and EOS = 1; decode([id]) returns the piece, so the pieces of a word concatenate to the word (what get_word_inds counts)."""
    model_max_length = 77

    def __init__(self):
        self.vocab = {"<bos>": 0, "<eos>": 1}
        self.words = ["<bos>", "<eos>"]

    def _id(self, piece):
        if piece not in self.vocab:
            self.vocab[piece] = len(self.words)
            self.words.append(piece)
        return self.vocab[piece]

    def encode(self, text):
        ids = [0]
        for w in text.split(" "):
            if not w:
                continue
            for piece in ([w[:4], w[4:]] if len(w) > 5 else [w]):
                ids.append(self._id(piece))
        return ids + [1]

    def decode(self, ids):
        if isinstance(ids, int):
            ids = [ids]
        return " ".join(self.words[int(i)] for i in ids)


# ------------------------------------------------------------------------------------------- the golden's protocol (tools/gen_golden_p2p.py)
G_H, G_D, G_NK, G_STEPS = 2, 8, 77, 4
G_LAYERS = (  # (place, is_cross, tokens): down_cross[2:4] and up_cross[:3] exist; self calls at and above the 16^2 rule
    ("down", False, 256), ("down", True, 256), ("down", True, 256), ("down", False, 289), ("down", True, 256), ("down", True, 256),
    ("mid", True, 256), ("up", True, 256), ("up", False, 256), ("up", True, 256), ("up", True, 256))
G_NMAX = 289
G_ROWS = (0, 17, 100, 255)          # rows recorded of every call (a 289-token call: the same rows and its last, below)
G_SELF_REPLACE = 0.5
G_THRESHOLD = 0.3
G_LATENT = (2, 4, 24, 40)
BASE_PROMPT = "a cat sits on the grass"
G_CONFIGS = {  # name -> (kind, prompts, key word of cross_replace_steps, extras)
    "store": ("store", [BASE_PROMPT, "a dog sits on the grass"], None),
    "replace": ("replace", [BASE_PROMPT, "a dog sits on the grass"], "dog"),
    "replace_split": ("replace", [BASE_PROMPT, "a giraffe sits on the grass"], "giraffe"),
    "refine": ("refine", [BASE_PROMPT, "a white cat sits on the grass"], "white"),
    "reweight": ("reweight", [BASE_PROMPT, BASE_PROMPT], "grass"),
    "reweight_refine": ("reweight_refine", [BASE_PROMPT, "a white cat sits on the grass"], "white"),
    "replace_blend": ("replace_blend", [BASE_PROMPT, "a dog sits on the grass"], "dog"),
    "replace3": ("replace", [BASE_PROMPT, "a dog sits on the grass", "a giraffe sits on the grass"], "dog"),
}
G_EQ = {"reweight": ("grass", (-2.0,)), "reweight_refine": ("white", (3.0,))}
G_BLEND_WORDS = ("cat", "dog")
G_MASK_WORDS = ["cat", "grass"]
OPERANDS = ("q_all", "k_all", "v_all", "k_cross", "v_cross")


def rows_of(N):
    return list(G_ROWS) + ([N - 1] if N - 1 not in G_ROWS else [])


def cross_steps(word):
    return {"default_": 0.5, word: (0., 1.)}


def call_inputs(g, step, layer, P):
    """(place, is_cross, q, k, v) of call `layer` of step `step` for P prompts: [2 P h, n, d] fp32 in the reference hook's (b h) layout.  The stored
    operands hold 3 + 3 samples ([u_0 u_1 u_2 c_0 c_1 c_2]); P = 2 takes [u_0 u_1 c_0 c_1].  Queries are scaled by a factor that differs per call."""
    place, is_cross, N = G_LAYERS[layer]
    f = 1.0 + 0.125 * ((3 * step + layer) % 5)
    samples = [0, 1, 3, 4] if P == 2 else [0, 1, 2, 3, 4, 5]
    sel = torch.tensor([s * G_H + h for s in samples for h in range(G_H)])
    q = g["q_all"][sel][:, :N] * f
    if is_cross:
        return place, True, q, g["k_cross"][sel], g["v_cross"][sel]
    return place, False, q, g["k_all"][sel][:, :N], g["v_all"][sel][:, :N]


def step_latent(g, step):
    return g["latent"] * (1.0 + 0.25 * step)


def load_golden(path):
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    for k in OPERANDS:
        g[k] = bf16_bits_to_f32(g[k])
    g["latent"] = torch.from_numpy(g["latent"])
    return g


def make_controller(name, pkg, tokenizer):
    """the controller of a golden configuration from a module with the reference's class names (the reference's own module, or the package)"""
    kind, prompts, word = G_CONFIGS[name]
    kw = {} if tokenizer is None else {"tokenizer": tokenizer}
    if kind == "store":
        return pkg.AttentionStore()
    args = (prompts, G_STEPS, cross_steps(word), G_SELF_REPLACE)
    if kind == "replace":
        return pkg.AttentionReplace(*args, **kw)
    if kind == "refine":
        return pkg.AttentionRefine(*args, **kw)
    if kind == "replace_blend":
        return pkg.AttentionReplace(*args, local_blend=pkg.LocalBlend(prompts, G_BLEND_WORDS, threshold=G_THRESHOLD, **kw), **kw)
    eq_word, eq_vals = G_EQ[name]
    eq = pkg.get_equalizer(prompts[1], eq_word, eq_vals, **kw)
    prev = pkg.AttentionRefine(*args, **kw) if kind == "reweight_refine" else None
    return pkg.AttentionReweight(*args, equalizer=eq, controller=prev, **kw)


# ------------------------------------------------------------------------------------------- kernel cases (CPU sensitivity test and GPU suite)
P2P_D, P2P_NK, P2P_N = (40, 64, 80, 160), (1, 8, 63, 64, 65, 77, 128), (1, 17, 64, 256, 1000)


def p2p_cases():
    """(D, Nk, N, H, B): each axis walked once against a rotation of the others (no cross product), H in {2, 3}, B in {4, 6}"""
    cases, i = [], 0
    for Nk in P2P_NK:
        cases.append((P2P_D[i % 4], Nk, P2P_N[(i + 1) % 5], 2 + i % 2, 4 + 2 * (i % 2)))
        i += 1
    for N in P2P_N:
        cases.append((P2P_D[i % 4], P2P_NK[(2 * i + 1) % 7], N, 2 + i % 2, 4 + 2 * (i % 2)))
        i += 1
    for D in P2P_D:
        cases.append((D, 77, 256 if D != 160 else 64, 2 + i % 2, 4 + 2 * (i % 2)))
        i += 1
    return cases


def case_id(c):
    return "D%d-Nk%d-N%d-H%d-B%d" % c


def case_operands(case, pad=16):
    """q in a padded buffer [B N, inner + pad], k | v packed in [B Nk, 2 inner + pad]; the pad columns hold NaN (never read).  Returns the bf16
    buffers, the strides and the float64 views."""
    D, Nk, N, H, B = case
    gen = torch.Generator().manual_seed(7000 + 13 * D + 5 * Nk + N + H + B)
    inner = H * D
    ldq, ldk = inner + pad, 2 * inner + pad
    q = torch.randn(B * N, ldq, generator=gen).bfloat16()
    q[:, inner:] = float("nan")
    kv = torch.randn(B * Nk, ldk, generator=gen).bfloat16()
    kv[:, 2 * inner:] = float("nan")
    qs, ks = (N * ldq, D, ldq), (Nk * ldk, D, ldk)
    Q = q.as_strided((B, H, N, D), qs + (1,), 0).to(F64)
    K = kv.as_strided((B, H, Nk, D), ks + (1,), 0).to(F64)
    V = kv.as_strided((B, H, Nk, D), ks + (1,), inner).to(F64)
    return q, kv, qs, ks, Q, K, V


def case_base(B):
    """[u ..., c_0, edited ...]: the conditional half's first sample is the base of the others"""
    P = B // 2
    return list(range(P)) + [P] * P


def case_edit(case, variant, tables=None):
    """(M or None, c, d) fp32 [B, ...] of an edit variant.  `dense`: random M (mixed signs), random c and d, some exactly 0 in both;
    `czero`: c = 0 and d = 1; `replace` / `refine` / `reweight`: the golden's tables (for Nk = 77), different per edited sample."""
    D, Nk, N, H, B = case
    gen = torch.Generator().manual_seed(9000 + 17 * D + 3 * Nk + N + B + len(variant))
    M = torch.zeros(B, Nk, Nk)
    c, d = torch.zeros(B, Nk), torch.ones(B, Nk)
    P = B // 2
    for e, b in enumerate(range(P + 1, B)):
        if variant == "dense":
            M[b] = torch.randn(Nk, Nk, generator=gen) * (1.0 / math.sqrt(Nk))
            c[b] = torch.randn(Nk, generator=gen)
            d[b] = torch.rand(Nk, generator=gen)
            z = torch.rand(Nk, generator=gen) < 0.2
            c[b][z] = 0.0
            d[b][z] = 0.0
        elif variant == "czero":
            M[b] = torch.randn(Nk, Nk, generator=gen)
        else:
            Mt, ct, dt = tables[variant]
            M[b] = Mt
            c[b] = ct * (0.5 if e else 1.0)
            d[b] = 1.0 - (1.0 - dt) * (0.5 if e else 1.0)
    if variant == "reweight":
        return None, c, d
    return M, c, d


def golden_tables(g):
    """(M, c, d) [77, 77] / [77] of the golden's replace (split word), refine and reweight configurations at a step where the gate is open"""
    t = {}
    a = torch.from_numpy(g["alpha.replace_split"])[0, 0].float()
    t["replace"] = (torch.from_numpy(g["mapper.replace_split"])[0].float(), a, 1 - a)
    mp = torch.from_numpy(g["mapper.refine"])[0].long()
    al = torch.from_numpy(g["alphas.refine"])[0].float()
    a = torch.from_numpy(g["alpha.refine"])[0, 0].float()
    M = torch.zeros(77, 77)
    M[mp % 77, torch.arange(77)] = 1.0
    t["refine"] = (M, al * a, 1 - al * a)
    a = torch.from_numpy(g["alpha.reweight"])[0, 0].float()
    eq = torch.from_numpy(g["equalizer.reweight"])[0].float()
    t["reweight"] = (torch.eye(77), eq * a, 1 - a)
    return t


# ------------------------------------------------------------------------------------------- blend cases
BLEND_CASES = [  # (id, S, (h, w), layers, kind, seed)
    ("64x64-5", 16, (64, 64), 5, "random", 1), ("16x16-1", 16, (16, 16), 1, "random", 2), ("24x40-5", 16, (24, 40), 5, "random", 3),
    ("empty-set", 16, (64, 64), 1, "empty", 4), ("zero-map", 16, (24, 40), 5, "zero", 5), ("exact", 16, (16, 16), 1, "exact", 6),
    ("at-max", 16, (64, 64), 1, "atmax", 7),
]
BLEND_NK, BLEND_C = 77, 4


def blend_case(case):
    """(maps, sets, thr, x).  `empty`: sample 1's token set is empty; `zero`: sample 0's maps are all zero; `exact`: one layer, one token, values
    that are multiples of 1/8 with maximum 1 and threshold 0.5 (normalised values exact in both precisions; 0.5 itself is not above 0.5); `atmax`:
    threshold 1.0, met exactly by the maximum pixel (x / x = 1 in both precisions, and 1 > 1 is false: the mask is empty)."""
    _, S, (h, w), L, kind, seed = case
    gen = torch.Generator().manual_seed(3000 + seed)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    blob = torch.stack([torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 18.0).reshape(-1) for cy, cx in ((5, 4), (9, 11))])     # [2, S S]
    maps = [(0.25 + torch.rand(2, S * S, BLEND_NK, generator=gen)) * blob[:, :, None] for _ in range(L)]
    sets = [[2, 5], [2, 70]]
    thr = 0.3
    if kind == "empty":
        sets = [[2, 5], []]
    if kind == "zero":
        for m in maps:
            m[0] = 0.0
    if kind == "exact":
        sets, thr = [[3], [3]], 0.5
        for b in range(2):
            maps[0][b, :, 3] = torch.randint(0, 9, (S * S,), generator=gen).float() / 8.0
            maps[0][b, 0, 3], maps[0][b, 5, 3], maps[0][b, 40, 3] = 1.0, 0.5, 0.0
    if kind == "atmax":
        thr = 1.0
    x = torch.randn(2, BLEND_C, h, w, generator=gen)
    return maps, sets, thr, x
