"""float64 statements of the adjoints that anyedit_amd/autodiff.py builds out of forward kernels, on bf16-rounded operands, each with the
absolute product its bound needs (the same expression with |dy| and |w|), the bounds themselves, and the case lists shared by
tests/test_tape_ref.py (CPU: the references against torch.autograd, a bf16-storage emulation of every route against the bounds) and
tests/test_hip_tape_adjoints.py (the tape on the GPU).

Layouts are the tape's: activations are channels-last rows [B*H*W, C]; a Linear weight is [N, K]; a conv weight is [Cout, Cin, 3, 3].

Bounds (tools/route_check.py):
  one GEMM / conv launch, bf16 result   2^-8 |ref| + 2^-16 sum|a||w| + 1e-30      (`launch_bound`)
  the same, fp32 result                 2^-20 |ref| + 2^-16 sum|a||w| + 1e-30     (`launch_bound(f32=True)`)
A route that stores bf16 more than once pays 2^-8 |stored value| per store and carries the bound of what it read (`store_bound`): the
stored value is within `carried` of `ref`, so its magnitude is at most |ref| + carried, and a round-to-nearest bf16 store moves it by at
most half a unit in the last place, 2^-8 of that (bf16 keeps 8 significant bits).  The fp32 additions in front of such a store (three for
a 2x2 block, one for a sum of two) are exact or within 2^-24 of the sum each, far inside the 2^-16 sum|a||w| the launches carry."""
import itertools

import torch
import torch.nn.functional as F

import norm_ref
import small_ref

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BF_EPS = 2.0 ** -8
F32_EPS = 2.0 ** -20
A_ACC = 2.0 ** -16
TINY = 1e-30


# =================================================================================================== operands
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def q(t):
    """round to bf16, keep as float64"""
    return t.to(F32).to(BF).to(F64)


def rnd(g, *shape, scale=1.0):
    return q(torch.randn(*shape, generator=g) * scale)


def to_nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def conv_out_hw(H, W, stride=1, up=False):
    Hv, Wv = (2 * H, 2 * W) if up else (H, W)
    return (Hv - 1) // stride + 1, (Wv - 1) // stride + 1


# =================================================================================================== bounds
def launch_bound(ref, absprod, f32=False):
    return (F32_EPS if f32 else BF_EPS) * ref.abs() + A_ACC * absprod + TINY


def store_bound(ref, carried):
    """one more bf16 store of a value that is within `carried` of `ref`"""
    return carried + BF_EPS * (ref.abs() + carried)


def one_rounding(ref):
    """an exact value (a sum of two bf16 numbers) stored to bf16 once: round to nearest moves it by at most half a unit in the last place,
    2^-8 |ref|; the fp32 addition in front of it is exact unless the exponents lie more than 16 apart, then it is within 2^-24 |ref|"""
    return (BF_EPS + 2.0 ** -23) * ref.abs() + TINY


# =================================================================================================== GEMM
def gemm_dx(dy, w):
    """y = a w^T  ->  dX = dY W [M, K]; a two-source K split takes the columns [:K1] and [K1:] of it"""
    return dy @ w, dy.abs() @ w.abs()


def gemm_dw(dy, a):
    """dW = dY^T A [N, K] (fp32 result)"""
    return dy.t() @ a, dy.abs().t() @ a.abs()


def gemm_db(dy):
    """db = column sums of dY (fp32 result); the 'product' is the sum of |dy|"""
    return dy.sum(0), dy.abs().sum(0)


def sum_of_launches(refs, absprods, f32=True):
    """parameter gradients of a weight used twice: each launch rounds to fp32, `add_param_grad` adds in fp32 (one more fp32 rounding of
    the total, 2^-24 relative, inside the 2^-20 term)"""
    ref = sum(refs)
    return ref, sum(launch_bound(r, p, f32) for r, p in zip(refs, absprods)) + F32_EPS * ref.abs()


def fanout_bounds(refs, absprods, fused):
    """a feeds GEMMs 1..3; the backward runs 3, 2, 1.
      step 3   g = bf16(dX3), stored by reference                       b = launch_bound(dX3)
      step 2   g = bf16(g + bf16(dX2)) out of place (ae_add_bf16)        b = store_bound(dX3 + dX2, b + launch_bound(dX2))
      step 1   fused:  g = bf16(g + dX1) in the GEMM's epilogue, dX1 still in fp32: only its accumulation error is carried
                                                                         b = store_bound(total, b + 2^-16 sum|dy1||w1|)
               un-fused: like step 2                                     b = store_bound(total, b + launch_bound(dX1))
    -> (total, bound)"""
    (r1, r2, r3), (p1, p2, p3) = refs, absprods
    b = launch_bound(r3, p3)
    b = store_bound(r3 + r2, b + launch_bound(r2, p2))
    total = r3 + r2 + r1
    b = store_bound(total, b + (A_ACC * p1 + TINY if fused else launch_bound(r1, p1)))
    return total, b


# =================================================================================================== 3x3 conv (padding 1)
def conv_forward(x_rows, w, B, H, W, stride=1, up=False, residual=None):
    """the forward in float64 (what torch.autograd differentiates in test_tape_ref.py)"""
    x = to_nchw(x_rows, B, H, W)
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = to_rows(F.conv2d(x, w, stride=stride, padding=1))
    return y if residual is None else y + residual


def _conv_t(dy_rows, w, B, Ho, Wo, Hv, Wv, stride):
    dy = to_nchw(dy_rows, B, Ho, Wo)
    op = (Hv - ((Ho - 1) * stride + 1), Wv - ((Wo - 1) * stride + 1))   # stride 2: 1 on an even side, 0 on an odd one
    return F.conv_transpose2d(dy, w, stride=stride, padding=1, output_padding=op)


def conv_dx(dy_rows, w, B, H, W, stride=1):
    """adjoint of the stride-1 / stride-2 conv: the transposed convolution back to H x W -> (ref rows [B*H*W, Cin], absprod).
    One launch stores it: `launch_bound`.  (On an odd map the stride-2 launch also computes a row / column at index H / W, which
    lies in the forward's zero padding; the tape drops it, so nothing of it enters the bound.)"""
    Ho, Wo = conv_out_hw(H, W, stride)
    return to_rows(_conv_t(dy_rows, w, B, Ho, Wo, H, W, stride)), to_rows(_conv_t(dy_rows.abs(), w.abs(), B, Ho, Wo, H, W, stride))


def conv_up_dx(dy_rows, w, B, H, W):
    """adjoint of conv(nearest_x2(x)): the stride-1 adjoint conv at 2H x 2W, stored to bf16, then the sums over 2x2 blocks, stored again.
    Each of the four values v_i of a block is within bnd_i = launch_bound(v_i) of its reference; their fp32 sum is within sum bnd_i of
    ref = sum v_i, and the pooled store pays 2^-8 of its magnitude:  bound = store_bound(ref, sum_i bnd_i).  -> (ref, bound)"""
    v = _conv_t(dy_rows, w, B, 2 * H, 2 * W, 2 * H, 2 * W, 1)
    av = _conv_t(dy_rows.abs(), w.abs(), B, 2 * H, 2 * W, 2 * H, 2 * W, 1)
    bv = launch_bound(v, av)

    def pool(t):
        return to_rows(t.reshape(B, -1, H, 2, W, 2).sum((3, 5)))
    ref = pool(v)
    return ref, store_bound(ref, pool(bv))


# =================================================================================================== layout adjoints
def concat_add(old, sl):
    """one side of the concat adjoint added to the gradient its tensor already has: exact sum, one rounding -> (ref, bound)"""
    ref = old + sl
    return ref, one_rounding(ref)


def nchw_adjoint(dy):
    """adjoint of rows_to_nchw: the transposition [B, C, H, W] -> rows, rounded to bf16 once (bit pattern known: compare exactly)"""
    return to_rows(dy).to(F32).to(BF)


# =================================================================================================== attention gate gradient
def attn_delta(qh, kh, vh, dO, scale):
    """[B, H, n, D] operands -> delta[b, h, q] = sum_d dO . Attn(q, K, V): its sum over heads and rows is d out / d gate_b"""
    p = torch.softmax(scale * qh @ kh.transpose(-1, -2), -1)
    return ((p @ vh) * dO).sum(-1)


def gate_grad(delta):
    """-> (ref [B], allowed difference): the quadrature bound derived in tests/test_hip_attention_training.py: 3 * 2e-2 * ||delta[b]||_2"""
    return delta.sum((1, 2)), 3 * 2e-2 * delta.flatten(1).norm(dim=1)


# =================================================================================================== a checkpointed segment
def ln_forward(x, gamma, beta, eps):
    return norm_ref.forward(x[:, None, :], gamma, beta, 1, eps, 0, False)["y"][:, 0, :]


def segment_forward(x, gamma, beta, w, r, eps):
    """LayerNorm -> GEMM (+ residual r) -> GEGLU in float64 -> (h, u, y)"""
    h = ln_forward(x, gamma, beta, eps)
    u = h @ w.t() + r
    return h, u, small_ref.ref_geglu(u)[0]


def segment_adjoint(x, gamma, beta, w, h, u, dy, eps):
    """The gradients that leave the segment y = geglu(LN(x) W^T + r): dx (bf16), dr (bf16), dW (fp32), each as (ref, bound).
    The adjoint is taken stage by stage AT the forward values the kernels stored (h, u: bf16), which is what the tape's backward reads
    (with exact h, u it is the gradient of the float64 forward: tests/test_tape_ref.py); each stage carries the bound of the gradient it
    read through its own absolute products and adds its own launch:
      du  = geglu_bwd(u, dy)         b_u = the bound of tests/small_ref.py (ref_geglu_bwd)
      dr  = du (stored by reference)                                     bound b_u
      dW  = du^T h, fp32             launch_bound(f32) with sum (|du| + b_u)^T |h|, + b_u^T |h|
      dh  = du W, bf16               store_bound(ref, b_u |W| + 2^-16 (|du| + b_u) |W|)
      dx  = LN_bwd(x, dh), bf16      the bound of tests/norm_ref.py at dh, + (1 + 2^-6) J(b_h), where J(b) = r (|g| b + mean(|g| b) +
                                     |xhat| mean(|g| b |xhat|)) is the absolute form of dx's linear dependence on dh; the 2^-6 covers what
                                     the kernel's own error terms (2^-8 |dx|, 2^-16 X^2 .., all of degree one in |dh|) add for the
                                     perturbation of dh: their coefficients stay below 2^-7 for |xhat|, r (|x| + |mu|) <= 8."""
    du, b_u = small_ref.ref_geglu_bwd(u, dy)
    au = du.abs() + b_u
    dw = du.t() @ h
    b_w = launch_bound(dw, au.t() @ h.abs(), f32=True) + b_u.t() @ h.abs()
    dh = du @ w
    b_h = store_bound(dh, b_u @ w.abs() + A_ACC * (au @ w.abs()) + TINY)
    nb = norm_ref.backward(x[:, None, :], gamma, beta, dh[:, None, :], 1, eps, 0, False)
    f = norm_ref.forward(x[:, None, :], gamma, beta, 1, eps, 0, False)
    xa, rs = f["xhat"][:, 0, :].abs(), f["rstd"]                       # rstd [M, 1]
    tb = gamma.to(F64).abs() * b_h
    J = rs * (tb + tb.mean(1, keepdim=True) + xa * (tb * xa).mean(1, keepdim=True))
    return dict(dx=(nb["dx"][:, 0, :], nb["bnd"][:, 0, :] + (1.0 + 2.0 ** -6) * J), dr=(du, b_u), dw=(dw, b_w))


SEGMENT = dict(M=7, C=64, F=72, eps=1e-5, seed=1950)


def segment_operands(c=SEGMENT):
    """-> x, gamma, beta, w [2F, C], r [M, 2F], dy [M, F]"""
    g = gen(c["seed"])
    M, C, F2 = c["M"], c["C"], 2 * c["F"]
    gamma, beta = (1.0 + 0.1 * torch.randn(C, generator=g)).float(), (0.1 * torch.randn(C, generator=g)).float()
    return rnd(g, M, C), gamma, beta, rnd(g, F2, C, scale=C ** -0.5), rnd(g, M, F2), rnd(g, M, c["F"])


# =================================================================================================== cases
def _prod(**kw):
    return [dict(zip(kw, v)) for v in itertools.product(*kw.values())]


def _seeded(cs, base):
    return [dict(c, seed=base + i) for i, c in enumerate(cs)]


_NK = [dict(N=8, K=8), dict(N=72, K=40), dict(N=320, K=328)]
_NK_W = [dict(N=8, K=8), dict(N=72, K=40), dict(N=768, K=64)]
_BHW = [dict(B=1, H=1, W=1), dict(B=2, H=3, W=5), dict(B=2, H=8, W=8)]
_BHW_UP = [dict(B=1, H=1, W=1), dict(B=2, H=3, W=5), dict(B=2, H=4, W=4)]
_HW_S2 = [dict(H=h, W=w) for h, w in ((2, 2), (4, 6), (8, 8), (1, 1), (3, 5), (7, 4))]

CASES = {
    "gemm_dx": _seeded([dict(M=m, **nk) for m in (1, 7, 200) for nk in _NK], 1000),
    "gemm_split": _seeded([dict(M=7, N=72, K1=k1, K2=k2, needs=n) for (k1, k2) in ((8, 8), (40, 72), (72, 8)) for n in ("a", "a2", "both")], 1100),
    "gemm_fanout": _seeded([dict(M=7, N=72, K=40), dict(M=200, N=320, K=328)], 1200),
    "gemm_dw": _seeded([dict(M=m, **nk) for m in (1, 4, 7, 8, 9, 33) for nk in _NK_W], 1300),
    "conv_s1": _seeded([dict(**s, Cin=ci, Cout=co) for s in _BHW for (ci, co) in ((8, 8), (64, 4), (72, 136), (8, 64))], 1400),
    "conv_up": _seeded([dict(**s, Cin=ci, Cout=co) for s in _BHW_UP for (ci, co) in ((64, 64), (72, 8))], 1500),
    "conv_s2": _seeded([dict(B=2, **s, Cin=ci, Cout=co) for s in _HW_S2 for (ci, co) in ((64, 64), (8, 72))], 1600),
    "concat": _seeded([dict(rows=r, ca=ca, cb=cb) for r in (1, 7, 130) for (ca, cb) in ((8, 8), (8, 72), (320, 8))], 1700),
    "rows_to_nchw": _seeded([dict(B=b, H=h, W=w, C=c, bf16=o) for (b, h, w, c) in ((1, 1, 1, 8), (2, 3, 5, 8), (2, 4, 4, 72)) for o in (0, 1)], 1800),
}


def gemm_operands(c, K=None):
    g = gen(c["seed"])
    K = K or c["K"]
    return rnd(g, c["M"], K), rnd(g, c["N"], K, scale=K ** -0.5), rnd(g, c["M"], c["N"])


def conv_operands(c, stride=1, up=False):
    """-> x rows, w [Cout, Cin, 3, 3], dy rows at the output resolution"""
    g = gen(c["seed"])
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    Ho, Wo = conv_out_hw(H, W, stride, up)
    return rnd(g, B * H * W, Cin), rnd(g, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5), rnd(g, B * Ho * Wo, Cout)
