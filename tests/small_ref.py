"""Seeded operands, references and element-wise bounds of the elementwise, sampler and training kernels (csrc/elementwise.hip, backward.hip,
gate.hip, expert_kv.hip), shared by tests/test_hip_small_kernels.py (GPU) and tests/test_small_ref.py (CPU: the references against the
sampler stand-ins and autograd, the bounds against deliberately wrong results).  torch on the CPU only; nothing here imports the extension.

Every reference is written from the formula in the kernel's header comment and the reference line it cites.  CASES names, per `extern "C"`
launch entry point of the four sources, the cases the GPU file runs.

Bound families (a = 2^-16, the project's fp32 accumulation constant of tests/norm_ref.py; 2^-8 = one bf16 rounding):
  (a) bit-exact      the sampler kernels (fp contraction off: the reference's un-fused fp32 expression order) and pure data movement:
                     the result has the bits of the fp32 stand-in / of the moved values.
  (b) bf16 result of a few fp32 operations          |got - ref| <= 2^-8 |ref| + 2^-22 sum|terms|
                     (fp32 results of a few operations, mse_grad: the second term alone)
  (c) the same through an approximated function     |got - ref| <= 2^-8 |ref| + a s,  s = the function's slope times the absolute argument terms
                     (SiLU 1.1, GELU 1.13, GELU' 0.8 (= max |GELU''|) plus its own value's terms; exp: the slope at the point, which is the result
                     itself — never more than the largest slope 1); fp32 results (gaussian_moments): a (|ref| + 1)
  (d) fp32 sums in a kernel-chosen order            |got - ref| <= a sum|terms| + 2^-20 |ref|
  (e) expert forward / dgrad (bf16)                 |got - ref| <= 2^-8 |ref| + a sum_k |x w|
  (f) AdamW                                         |got - ref| <= a (|p| + lr) per step taken
"""
import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
A = 2.0 ** -16
BF_EPS = 2.0 ** -8
TINY = 1e-30
GRID_WRAP = 4096 * 256 + 257       # work items of one pass of a 4096-block grid of 256 threads, and a ragged rest
MSE_WRAP = 1024 * 256 + 257        # ae_mse_f32 caps its grid at 1024 blocks
SLOPE_SILU, SLOPE_GELU, CURV_GELU = 1.1, 1.13, 0.8


class BoundFailure(Exception):
    pass


# =================================================================================================== sampler stand-ins
class SamplerStandIns:
    """torch statements of the sampler kernels' documented arithmetic (csrc/elementwise.hip: DdimArgs ... dpm_adaptive_err_kernel)."""

    @staticmethod
    def _guided(eps, n_like, branches, s0, s1=0.0):
        parts = eps.reshape(branches, *n_like.shape)
        if branches == 1:
            return parts[0]
        if branches == 2:                                                   # [uncond, cond]
            return parts[0] + s0 * (parts[1] - parts[0])
        et, ei, eu = parts                                                   # [text, image, uncond]
        return eu + s0 * (et - ei) + s1 * (ei - eu)

    @classmethod
    def ddim_step(cls, x, eps, coeffs, branches, s0=1.0, s1=0.0, noise=None, temperature=1.0, want_pred_x0=True, want_e=False):
        s1m, sat, sap, dirc, sig = (torch.tensor(c, dtype=torch.float32) for c in coeffs)
        e = cls._guided(eps, x, branches, s0, s1)
        px0 = (x - s1m * e) / sat
        nz = sig * (noise if noise is not None else torch.zeros_like(x)) * temperature
        x_prev = sap * px0 + dirc * e + nz
        return (x_prev, px0, e) if want_e else (x_prev, px0)

    @classmethod
    def ddim_encode_step(cls, x, eps, cx, ce, branches=1, scale=1.0):
        e = cls._guided(eps, x, branches, scale)
        return torch.tensor(cx, dtype=torch.float32) * x + torch.tensor(ce, dtype=torch.float32) * e

    @staticmethod
    def plms_combine(e_t, old_eps):
        o = list(old_eps[::-1][:3])
        if len(o) == 1:
            return (3.0 * e_t - o[0]) / 2.0
        if len(o) == 2:
            return ((23.0 * e_t - 16.0 * o[0]) + 5.0 * o[1]) / 12.0
        return (((55.0 * e_t - 59.0 * o[0]) + 37.0 * o[1]) - 9.0 * o[2]) / 24.0

    @staticmethod
    def plms_combine_first(e_t, e_t_next):
        return (e_t + e_t_next) / 2.0

    @staticmethod
    def mask_blend(img, x0, noise, mask, sqrt_ac, sqrt_one_minus_ac, ip2p_order=False):
        q = torch.tensor(sqrt_ac, dtype=torch.float32) * x0 + torch.tensor(sqrt_one_minus_ac, dtype=torch.float32) * noise
        m = mask.float()
        return img * m + q * (1.0 - m) if ip2p_order else q * m + (1.0 - m) * img

    @staticmethod
    def q_sample(x0, noise, sqrt_ac_t, sqrt_one_minus_ac_t):
        shape = (-1,) + (1,) * (x0.dim() - 1)
        return sqrt_ac_t.reshape(shape) * x0 + sqrt_one_minus_ac_t.reshape(shape) * noise

    @staticmethod
    def dpm_multistep(x, model_out, branches, scale, sigma_s, alpha_s, predict_x0=True, v_param=False, m_prev=None, update=None, want_m=True):
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        parts = model_out.reshape(branches, *x.shape)
        conv = (lambda o: f(alpha_s) * o + f(sigma_s) * x) if v_param else (lambda o: o)
        e = conv(parts[0])
        if branches == 2:
            e = e + f(scale) * (conv(parts[1]) - e)
        m = (x - f(sigma_s) * e) / f(alpha_s) if predict_x0 else e
        xn = None
        if update is not None:
            a, b, c, inv_r0 = update
            xn = f(a) * x - f(b) * m
            if m_prev is not None:
                xn = xn - f(c) * (f(inv_r0) * (m - m_prev))
        return (m if want_m else None), xn

    @staticmethod
    def lincomb(terms, out=None):
        acc = None
        for t, c in terms:
            if t is None:
                continue
            term = torch.tensor(float(c), dtype=torch.float32) * t
            acc = term if acc is None else acc + term
        return acc

    @staticmethod
    def dpm_adaptive_err(x_lower, x_higher, x_prev, atol, rtol):
        delta = torch.max(torch.full_like(x_lower, atol), rtol * torch.max(x_lower.abs(), x_prev.abs()))
        d = ((x_higher - x_lower) / delta).reshape(x_lower.shape[0], -1)
        return torch.sqrt((d * d).mean(1))


# =================================================================================================== operands
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def randn(g, *shape, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def c32(v):
    """a python float holding the fp32 value the C ABI receives"""
    return float(torch.tensor(float(v), dtype=F32))


def _s(v):
    return torch.tensor(float(v), dtype=F32)


# =================================================================================================== checks
def check_elements(got, ref, bnd, what):
    """every element of `got` within `bnd` of `ref`; returns the worst error / bound"""
    got = got.to(F64)
    if got.shape != ref.shape:
        raise BoundFailure(f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}")
    if not torch.isfinite(got).all():
        raise BoundFailure(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values")
    if isinstance(bnd, float):
        bnd = torch.full_like(ref, bnd)
    q = (got - ref.to(F64)).abs() / bnd
    ratio = float(q.max()) if q.numel() else 0.0
    if ratio > 1.0:
        i = int(q.flatten().argmax())
        raise BoundFailure(f"{what}: flat element {i} got {float(got.flatten()[i]):.9g} ref {float(ref.flatten()[i]):.9g} bound "
                           f"{float(bnd.flatten()[i]):.3g} (ratio {ratio:.2f}); {int((q > 1).sum())} of {q.numel()} elements fail")
    return ratio


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def check_bits(got, ref, what):
    """family (a): same shape, dtype and bits (so -0 against +0 and a NaN payload count)"""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        raise BoundFailure(f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(ref.shape)} {ref.dtype}")
    ne = _bits(got) != _bits(ref)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        raise BoundFailure(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits, the first at flat index {i}: "
                           f"{float(got.flatten()[i])!r} against {float(ref.flatten()[i])!r}")
    return 0.0


def bound_b(ref, terms, bf16_out=True):
    return (BF_EPS * ref.abs() if bf16_out else 0.0) + 2.0 ** -22 * terms + TINY


def bound_c(ref, slope_args):
    return BF_EPS * ref.abs() + A * slope_args + TINY


def bound_c32(ref):
    return A * (ref.abs() + 1.0)


def bound_d(ref, terms):
    return A * terms + 2.0 ** -20 * ref.abs() + TINY


def bound_e(ref, terms):
    return BF_EPS * ref.abs() + A * terms + TINY


def bound_f(p, lr, steps=1):
    return steps * A * (p.abs() + lr)


# =================================================================================================== (a) samplers, fp32, flat
def ref_guided(eps, n, branches, s0, s1=0.0):
    """ddim.py:211-212 ([uncond, cond]) / global_tool.py:172-177 ([text, image, uncond]) on `branches` stacked flat predictions"""
    p = eps.reshape(-1)
    if branches == 1:
        return p[:n]
    if branches == 2:
        eu, ec = p[:n], p[n:2 * n]
        return eu + _s(s0) * (ec - eu)
    et, ei, eu = p[:n], p[n:2 * n], p[2 * n:3 * n]
    return eu + _s(s0) * (et - ei) + _s(s1) * (ei - eu)


def ref_ddim_step(x, eps, coeffs, branches, s0=1.0, s1=0.0, noise=None, temperature=1.0):
    """ddim.py:235, 246, 247, 250 -> (x_prev, pred_x0, e), each of x's shape"""
    s1m, sat, sap, dirc, sig = (_s(c) for c in coeffs)
    xf = x.reshape(-1)
    e = ref_guided(eps, xf.numel(), branches, s0, s1)
    px0 = (xf - s1m * e) / sat
    dir_ = dirc * e
    nz = sig * (noise.reshape(-1) if noise is not None else torch.zeros_like(xf)) * _s(temperature)
    xp = sap * px0 + dir_ + nz
    return xp.reshape(x.shape), px0.reshape(x.shape), e.reshape(x.shape).clone()


def ref_ddim_encode_step(x, eps, cx, ce, branches=1, scale=1.0):
    xf = x.reshape(-1)
    e = ref_guided(eps, xf.numel(), branches, scale) if branches == 2 else eps.reshape(-1)[:xf.numel()]
    return (_s(cx) * xf + _s(ce) * e).reshape(x.shape)


def ref_plms(e, olds_newest_first, order):
    """plms.py:226-240; order 0 is the pseudo improved Euler mean with the prediction at the next timestep"""
    o = olds_newest_first
    if order == 0:
        return (e + o[0]) / 2.0
    if order == 1:
        return (3.0 * e - o[0]) / 2.0
    if order == 2:
        return ((23.0 * e - 16.0 * o[0]) + 5.0 * o[1]) / 12.0
    return (((55.0 * e - 59.0 * o[0]) + 37.0 * o[1]) - 9.0 * o[2]) / 24.0


def ref_plms_combine(e_t, old_eps):
    """the product's calling convention: the history newest last, the newest three used"""
    o = list(old_eps[::-1][:3])
    return ref_plms(e_t, o, len(o))


def ref_mask_blend(img, x0, noise, mask, sa, s1, ip2p_order=False):
    """ddim.py:154-157 with q_sample ddpm.py:356-359; mask broadcast against [B, C, H, W]"""
    m = mask.float().expand(img.shape)
    q = _s(sa) * x0 + _s(s1) * noise
    one = torch.ones((), dtype=F32)
    return img * m + q * (one - m) if ip2p_order else q * m + (one - m) * img


def ref_q_sample(x0, noise, sa, s1):
    B = x0.shape[0]
    per = x0.numel() // B
    b = torch.arange(x0.numel()) // per
    return (sa[b] * x0.reshape(-1) + s1[b] * noise.reshape(-1)).reshape(x0.shape)


def ref_dpm_multistep(x, out, branches, scale, sigma_s, alpha_s, predict_x0=True, v_param=False, m_prev=None, update=None):
    """-> (m, x_next or None); dpm_solver.py:246-316, 352-365, 469-513, 723-777"""
    xf, o = x.reshape(-1), out.reshape(-1)
    n = xf.numel()
    al, sg = _s(alpha_s), _s(sigma_s)
    e = o[:n]
    if v_param:
        e = al * e + sg * xf
    if branches == 2:
        ec = o[n:2 * n]
        if v_param:
            ec = al * ec + sg * xf
        e = e + _s(scale) * (ec - e)
    m = (xf - sg * e) / al if predict_x0 else e.clone()
    xn = None
    if update is not None:
        a, b, c, inv_r0 = (_s(v) for v in update)
        xn = a * xf - b * m
        if m_prev is not None:
            D = inv_r0 * (m - m_prev.reshape(-1))
            xn = xn - c * D
        xn = xn.reshape(x.shape)
    return m.reshape(x.shape), xn


# =================================================================================================== (a) data movement
def ref_transpose(x, Xpad, out_dtype):
    """x [B, X, Y] -> [B, Y, Xpad], zero for X <= x < Xpad, converted once"""
    B, X, Y = x.shape
    out = torch.zeros(B, Y, Xpad, dtype=out_dtype)
    out[:, :, :X] = x.transpose(1, 2).to(out_dtype)
    return out


def ref_im2col3x3_c8(rows, B, H, W):
    """rows [B*H*W, 8] -> [B*H*W, 128]: nine taps (3 ky + kx) of 8 channels, zero outside the image, 56 zero columns"""
    x = rows.reshape(B, H, W, 8)
    xp = torch.zeros(B, H + 2, W + 2, 8, dtype=rows.dtype)
    xp[:, 1:-1, 1:-1] = x
    out = torch.zeros(B, H, W, 128, dtype=rows.dtype)
    for tap in range(9):
        out[..., 8 * tap:8 * tap + 8] = xp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W]
    return out.reshape(B * H * W, 128)


def ref_patchify(x, P):
    """x [B, Cin, H, W] fp32 -> [B (H/P) (W/P), Cin P P] bf16, K order (c, ky, kx)"""
    B, C, H, W = x.shape
    t = x.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(B * (H // P) * (W // P), C * P * P).to(BF)


def window_index(B, H, W, ws):
    """image row of every window row, -1 for padding (image_encoder.py:243-264)"""
    nH, nW = (H + ws - 1) // ws, (W + ws - 1) // ws
    b, jh, jw, wy, wx = torch.meshgrid(torch.arange(B), torch.arange(nH), torch.arange(nW), torch.arange(ws), torch.arange(ws), indexing="ij")
    yy, xx = jh * ws + wy, jw * ws + wx
    img = (b * H + yy) * W + xx
    img[(yy >= H) | (xx >= W)] = -1
    return img.reshape(-1)


def ref_window_partition(x, B, H, W, ws):
    idx = window_index(B, H, W, ws)
    out = torch.zeros(idx.numel(), x.shape[1], dtype=x.dtype)
    out[idx >= 0] = x[idx[idx >= 0]]
    return out


def ref_window_unpartition(win, B, H, W, ws):
    idx = window_index(B, H, W, ws)
    out = torch.zeros(B * H * W, win.shape[1], dtype=win.dtype)
    out[idx[idx >= 0]] = win[idx >= 0]
    return out


def ref_nearest2x(x, B, H, W):
    C = x.shape[1]
    return x.reshape(B, H, W, C).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(-1, C)


# =================================================================================================== (b), (c): float64 and bounds
def ref_axpy(a, b, alpha=1.0):
    al = float(_s(alpha))
    ref = a.to(F64) + al * b.to(F64)
    return ref, bound_b(ref, a.to(F64).abs() + abs(al) * b.to(F64).abs())


def ref_add_bcast(x, p):
    pp = p.to(F64).reshape(-1).repeat(x.numel() // p.numel()).reshape(x.shape)
    ref = x.to(F64) + pp
    return ref, bound_b(ref, x.to(F64).abs() + pp.abs())


def ref_split(dy, ca, old_a=None, old_b=None):
    """-> ((ref_a, bnd_a), (ref_b, bnd_b)); without an old value the slice is moved (family a: bound None)"""
    out = []
    for sl, old in ((dy[:, :ca], old_a), (dy[:, ca:], old_b)):
        if old is None:
            out.append((sl.contiguous(), None))
        else:
            ref = sl.to(F64) + old.to(F64)
            out.append((ref, bound_b(ref, sl.to(F64).abs() + old.to(F64).abs())))
    return out


def ref_sumpool2x2(x, B, H, W):
    """x [B 2H 2W, C] -> [B H W, C]: the adjoint of the nearest x2 upsample (openaimodel.py:108-118)"""
    C = x.shape[1]
    t = x.to(F64).reshape(B, H, 2, W, 2, C)
    ref = t.sum((2, 4)).reshape(-1, C)
    return ref, bound_b(ref, t.abs().sum((2, 4)).reshape(-1, C))


def ref_mean2x2(x, B, H, W):
    """AvgPool2d(2, 2) on channels-last rows: an odd last row / column is dropped (openaimodel.py:154-155)"""
    C = x.shape[1]
    Ho, Wo = H // 2, W // 2
    t = x.to(F64).reshape(B, H, W, C)[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C)
    ref = t.mean((2, 4)).reshape(-1, C)
    return ref, bound_b(ref, t.abs().mean((2, 4)).reshape(-1, C))


def ref_silu(x):
    z = x.to(F64)
    ref = z * torch.sigmoid(z)
    return ref, bound_c(ref, SLOPE_SILU * z.abs())


def ref_scale_shift(x, emb, B, HW, silu):
    """openaimodel.py:264-268: act(x (1 + scale) + shift); emb [B, 2C] = scale | shift"""
    C = x.shape[1]
    e = emb.to(F64)
    sc, sh = e[:, :C].repeat_interleave(HW, 0), e[:, C:].repeat_interleave(HW, 0)
    xx = x.to(F64)
    z = xx * (1.0 + sc) + sh
    terms = xx.abs() * (1.0 + sc.abs()) + sh.abs()
    if not silu:
        return z, bound_b(z, terms)
    ref = z * torch.sigmoid(z)
    return ref, bound_c(ref, SLOPE_SILU * terms)


def gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def gelu_grad64(g):
    return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def ref_geglu(h):
    """attention.py:49-57: h = [a | g] -> a gelu(g), exact-erf GELU"""
    F = h.shape[1] // 2
    a, g = h.to(F64)[:, :F], h.to(F64)[:, F:]
    ref = a * gelu64(g)
    return ref, bound_c(ref, SLOPE_GELU * a.abs() * g.abs())


def ref_geglu_bwd(h, dy):
    """-> (dh [M, 2F], bound): da = dy gelu(g), dg = dy a gelu'(g)"""
    F = h.shape[1] // 2
    a, g, d = h.to(F64)[:, :F], h.to(F64)[:, F:], dy.to(F64)
    da, dg = d * gelu64(g), d * a * gelu_grad64(g)
    ref = torch.cat([da, dg], 1)
    bnd = torch.cat([bound_c(da, SLOPE_GELU * d.abs() * g.abs()), bound_c(dg, (d * a).abs() * (CURV_GELU * g.abs() + SLOPE_GELU))], 1)
    return ref, bnd


def ref_softmax_rows(S, scale):
    """softmax(scale S) over the last dim; the argument of exp is scale (S - max): terms scale (|S| + |max|)"""
    z = S.to(F64) * float(_s(scale))
    mx = z.max(-1, keepdim=True).values
    ref = torch.softmax(z, -1)
    args = z.abs() + mx.abs()
    return ref, BF_EPS * ref + A * ref * (1.0 + args) + 2.0 ** -125


def ref_gaussian(moments, noise=None):
    """distributions.py:25-37 -> dict(z, mean, logvar, std) float64; mean and the clamped logvar are moved (family a)"""
    B, C2 = moments.shape[:2]
    m = moments.to(F64)
    mean, logvar = m[:, :C2 // 2], m[:, C2 // 2:].clamp(-30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    z = mean + std * noise.to(F64) if noise is not None else mean.clone()
    return dict(z=z, mean=mean, logvar=logvar, std=std)


def ref_timestep_embedding(t, dim, max_period=10000.0):
    """util.py:154-174, [cos, sin] order, a zero column for an odd dim"""
    half = dim // 2
    freqs = torch.exp(-math.log(float(_s(max_period))) * torch.arange(half, dtype=F64) / half)
    args = t.to(F32).to(F64)[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], -1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], -1)
    return emb


TIMESTEP_TOL = 2e-4


# =================================================================================================== (d) sums
def ref_mse(a, b):
    d = a.to(F32).to(F64) - b.to(F32).to(F64)
    ref = (d * d).mean().reshape(())
    return ref, bound_d(ref, ref.abs())


def ref_mse_grad(pred, target, loss_scale=1.0):
    coef = 2.0 * float(_s(loss_scale)) / pred.numel()
    ref = coef * (pred.to(F64) - target.to(F64))
    return ref, bound_b(ref, coef * (pred.to(F64).abs() + target.to(F64).abs()), bf16_out=False)


def ref_rowsum(x):
    ref = x.to(F64).sum(1)
    return ref, bound_d(ref, x.to(F64).abs().sum(1))


def ref_colsum(x):
    ref = x.to(F64).sum(0)
    return ref, bound_d(ref, x.to(F64).abs().sum(0))


def ref_lincomb(terms):
    ts = [(t.to(F64), float(_s(c))) for t, c in terms if t is not None]
    ref = sum(c * t for t, c in ts)
    return ref, bound_d(ref, sum(abs(c) * t.abs() for t, c in ts))


def adaptive_delta(xl, xp, atol, rtol):
    """-> (delta, r) float64: r = rtol max(|x_lower|, |x_prev|), delta = max(atol, r)  (dpm_solver.py:925)"""
    r = float(_s(rtol)) * torch.maximum(xl.to(F64).abs(), xp.to(F64).abs())
    return torch.clamp(r, min=float(_s(atol))), r


def ref_dpm_adaptive_err(xl, xh, xp, atol, rtol):
    """dpm_solver.py:925-927, per sample; sqrt halves the relative error of the mean (a sum|terms| = a ref^2)"""
    B = xl.shape[0]
    delta, _ = adaptive_delta(xl, xp, atol, rtol)
    v = ((xh.to(F64) - xl.to(F64)) / delta).reshape(B, -1)
    ref = torch.sqrt((v * v).mean(1))
    return ref, 0.5 * A * ref + 2.0 ** -20 * ref + TINY


def ref_scatter_add_rows(src, code, dst):
    ref, terms = dst.to(F64).clone(), dst.to(F64).abs()
    for b in range(src.shape[0]):
        ref[int(code[b])] += src[b].to(F64)
        terms[int(code[b])] += src[b].to(F64).abs()
    return ref, bound_d(ref, terms)


def ref_relpos(q, Rh, Rw, qH, qW):
    """image_encoder.py:349-355.  q [B, qH qW, heads, D] -> rel_h [B heads, qH qW, kH], rel_w [B heads, qH qW, kW], each with its bound"""
    B, N, Hh, D = q.shape
    r = q.to(F64).reshape(B, qH, qW, Hh, D)
    out = []
    for eq, R in (("byxhc,ykc->bhyxk", Rh.to(F64)), ("byxhc,xkc->bhyxk", Rw.to(F64))):
        ref = torch.einsum(eq, r, R).reshape(B * Hh, N, R.shape[1])
        terms = torch.einsum(eq, r.abs(), R.abs()).reshape(B * Hh, N, R.shape[1])
        out.append((ref, bound_d(ref, terms)))
    return out


# =================================================================================================== gate
def gate_forward64(te, code, Wg, bg):
    """logits = <task_emb[clamp(code)], Wg[e]> + bg[e] -> (logits, sum|terms|) float64"""
    c = code.long().clamp(0, te.shape[0] - 1)
    t = te.to(F64)[c]
    terms = t[:, None, :] * Wg.to(F64)[None]
    b = bg.to(F64) if bg is not None else torch.zeros(Wg.shape[0], dtype=F64)
    return terms.sum(-1) + b, terms.abs().sum(-1) + b.abs()


def first_argmax(v):
    E = v.shape[-1]
    return torch.where(v == v.max(-1, keepdim=True).values, torch.arange(E), torch.tensor(E)).min(-1).values


def ref_task_gate(te, code, Wg, bg):
    """-> dict(probs, bnd [B, E], top1 [B] (lowest index on ties), top1_prob, bnd_top1 [B])"""
    logits, labs = gate_forward64(te, code, Wg, bg)
    p = torch.softmax(logits, -1)
    dl = bound_d(logits, labs)
    bnd = p * (dl + (p * dl).sum(-1, keepdim=True) + A) + 2.0 ** -125
    top1 = first_argmax(logits)
    ar = torch.arange(p.shape[0])
    return dict(logits=logits, probs=p, bnd=bnd, top1=top1, top1_prob=p[ar, top1], bnd_top1=bnd[ar, top1])


def gate_dlogit(probs, top1, dgate):
    """gate.hip: dlogit[b, e] = dg_b g_b ((e == top1_b) - p[b, e]),  g_b = p[b, top1_b]"""
    p = probs.to(F64)
    B, E = p.shape
    g = p[torch.arange(B), top1.long()]
    oh = torch.nn.functional.one_hot(top1.long(), E).to(F64)
    return (dgate.to(F64) * g)[:, None] * (oh - p)


def ref_task_gate_bwd(probs, top1, dgate, Wg):
    dl = gate_dlogit(probs, top1, dgate)
    ref = dl @ Wg.to(F64)
    return ref, bound_d(ref, dl.abs() @ Wg.to(F64).abs())


def ref_task_gate_wgrad(probs, top1, dgate, te, code):
    dl = gate_dlogit(probs, top1, dgate)
    t = te.to(F64)[code.long().clamp(0, te.shape[0] - 1)]
    dW, db = dl.t() @ t, dl.sum(0)
    return (dW, bound_d(dW, dl.abs().t() @ t.abs())), (db, bound_d(db, dl.abs().sum(0)))


# =================================================================================================== experts
def _expert_w(W, experts):
    return W.to(BF).to(F64)[experts.long().clamp(0, W.shape[0] - 1)]       # [B, N, Dc], the masters rounded to bf16 as the kernels do


def ref_expert_fwd(x, W, experts, T):
    """expert_kv.hip: kv[b] = ip_rows[b] @ bf16(W[e_b])^T"""
    B = x.shape[0] // T
    xs, w = x.to(F64).reshape(B, T, -1), _expert_w(W, experts)
    ref = torch.einsum("btk,bnk->btn", xs, w).reshape(B * T, -1)
    return ref, bound_e(ref, torch.einsum("btk,bnk->btn", xs.abs(), w.abs()).reshape(B * T, -1))


def ref_expert_dgrad(dy, W, experts, T):
    B = dy.shape[0] // T
    d, w = dy.to(F64).reshape(B, T, -1), _expert_w(W, experts)
    ref = torch.einsum("btn,bnk->btk", d, w).reshape(B * T, -1)
    return ref, bound_e(ref, torch.einsum("btn,bnk->btk", d.abs(), w.abs()).reshape(B * T, -1))


def ref_expert_wgrad(dy, x, experts, T, E):
    B = dy.shape[0] // T
    d, xs = dy.to(F64).reshape(B, T, -1), x.to(F64).reshape(B, T, -1)
    oh = torch.nn.functional.one_hot(experts.long().clamp(0, E - 1), E).to(F64)
    ref = torch.einsum("be,btn,btk->enk", oh, d, xs)
    return ref, bound_d(ref, torch.einsum("be,btn,btk->enk", oh, d.abs(), xs.abs()))


# =================================================================================================== AdamW
def ref_adamw(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    """One torch.optim.AdamW step in float64 on the fp32 hyper-parameters the C ABI receives -> (p, m, v)"""
    lr, b1, b2, eps, wd, gs = (c32(c) for c in (lr, betas[0], betas[1], eps, weight_decay, grad_scale))
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    g = g * gs
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


# =================================================================================================== case data shared by CPU and GPU tests
def gate_case(c):
    """-> (task_emb [n_tasks, Dt], code [4 or B] int64, Wg [E, Dt], bg or None): logits of spread ~50, codes past both ends"""
    g = gen(c["seed"])
    n_tasks, Dt, E = c.get("n_tasks", 6), c["Dt"], c["E"]
    te = randn(g, n_tasks, Dt)
    Wg = randn(g, E, Dt, scale=50.0 / math.sqrt(Dt))
    bg = randn(g, E, scale=5.0) if c["bg"] else None
    code = torch.tensor(c.get("code", [-1, 0, n_tasks - 1, n_tasks + 3]), dtype=torch.int64)
    if c.get("tie"):
        lo, hi = c["tie"]
        Wg[lo] = te[0] * (400.0 / float((te[0] * te[0]).sum()))       # samples of task 0 (codes -1 and 0): both rows win, equally
        Wg[hi] = Wg[lo]
        if bg is not None:
            bg[hi] = bg[lo]
    return te, code, Wg, bg


def adaptive_case(c):
    g = gen(c["seed"])
    B, n = c["B"], c["n"]
    xl, xp = randn(g, B, n, scale=0.3), randn(g, B, n, scale=0.3)
    xh = xl + randn(g, B, n, scale=0.01)
    return xl, xh, xp, c["atol"], c["rtol"]


def expert_ids(c):
    B, E = c["B"], c["E"]
    kind = c.get("ids", "spread")
    if kind == "one":
        return torch.full((B,), E - 1, dtype=torch.int64)
    if kind == "clamp":
        return torch.tensor(([-1, E + 2] * B)[:B], dtype=torch.int64)
    return torch.arange(B, dtype=torch.int64) % E


def _prod(**kw):
    out = [{}]
    for k, vs in kw.items():
        out = [dict(o, **{k: v}) for o in out for v in vs]
    return out


_EXPERT_SHAPES = [(1, 1, 16, 4, 1), (3, 8, 32, 260, 2), (2, 5, 64, 768, 3), (32, 8, 16, 8, 4), (2, 4, 80, 4096, 2)]
_EXPERT = ([dict(B=b, T=t, N=n, Dc=d, E=e, seed=90 + i) for i, (b, t, n, d, e) in enumerate(_EXPERT_SHAPES)]
           + [dict(B=3, T=8, N=32, Dc=260, E=2, ids="one", seed=96), dict(B=4, T=5, N=64, Dc=768, E=3, ids="clamp", seed=97)])
_RELPOS = ([dict(D=D, qH=4, qW=5, kH=kh, kW=kw, route=r, seed=40 + i)
            for i, (r, D) in enumerate([("mfma", 16), ("mfma", 48), ("mfma", 80), ("mfma", 96), ("line", 40), ("line", 72), ("generic", 12)])
            for kh, kw in ((8, 14), (14, 7), (7, 17), (17, 8))]
           + [dict(D=80, qH=65, qW=2, kH=7, kW=8, route="mfma", seed=48), dict(D=40, qH=65, qW=2, kH=7, kW=8, route="generic", seed=49)])
_TRANSPOSE = [dict(X=x, Y=y, Xpad=p, in_bf16=i, out_bf16=o) for (x, y, p) in ((20, 63, 24), (31, 33, 40), (32, 32, 33), (1, 1, 8), (33, 1, 33))
              for i in (0, 1) for o in (0, 1)]
_WINDOW = [dict(H=h, W=w, ws=s, C=c) for (h, w, s) in ((5, 9, 4), (14, 14, 14), (15, 13, 7)) for c in (8, 24)] + [dict(H=1025, W=1024, ws=4, C=8, B=1, wrap=True)]
_GATE_FWD = ([dict(E=e, Dt=d, bg=bg, seed=70 + 7 * e + d % 5 + bg) for e in (1, 2, 11, 64) for d in (1, 48, 768) for bg in (0, 1)]
             + [dict(E=11, Dt=48, bg=1, tie=(3, 7), seed=69)])
_GATE_BWD = [dict(E=11, Dt=d, bg=1, n_tasks=6, code=[3, 0, 3, 5, 0], seed=80 + d % 7) for d in (48, 300)]
_W = GRID_WRAP

CASES = {
    # ---- elementwise.hip
    "ae_transpose_last2": _TRANSPOSE,
    "ae_concat_channels_bf16": [dict(Ca=8, Cb=16, rows=5), dict(Ca=320, Cb=640, rows=5), dict(Ca=8, Cb=8, rows=5), dict(Ca=8, Cb=8, rows=(_W + 1) // 2, wrap=True)],
    "ae_split_channels_bf16": ([dict(Ca=ca, Cb=cb, rows=5, acc=acc, want=w) for (ca, cb) in ((8, 16), (320, 640), (8, 8)) for acc in (0, 1)
                                for w in ("ab", "a", "b")] + [dict(Ca=8, Cb=8, rows=(_W + 1) // 2, acc=1, want="ab", wrap=True)]),
    "ae_im2col3x3_c8_bf16": [dict(B=2, H=16, W=16), dict(B=1, H=5, W=7), dict(B=12, H=64, W=64), dict(B=1, H=257, W=256, wrap=True)],
    "ae_timestep_embedding": _prod(dim=[2, 7, 320, 321], kind=["i64", "f32"], max_period=[10000.0, 100.0]),
    "ae_ddim_step_f32": _prod(branches=[1, 2, 3], noise=[0, 1], want_e=[0, 1], n=[3 * 4 * 5 * 7]) + [dict(branches=3, noise=1, want_e=1, n=_W, wrap=True)],
    "ae_ddim_encode_step_f32": [dict(branches=1, n=420), dict(branches=2, n=420), dict(branches=2, n=_W, wrap=True)],
    "ae_plms_combine_f32": [dict(hist=h, n=420) for h in (0, 1, 2, 3, 4)] + [dict(hist=4, n=_W, wrap=True)],       # hist 0: plms_combine_first
    "ae_mask_blend_f32": (_prod(order=[0, 1], mask=["B1", "11", "BC"], B=[3], C=[4], H=[5], W=[7])
                          + [dict(order=0, mask="B1", B=3, C=3, H=1, W=_W // 9, wrap=True)]),
    "ae_q_sample_f32": [dict(B=3, per=257), dict(B=3, per=_W // 3, wrap=True)],
    "ae_dpm_multistep_f32": (_prod(branches=[1, 2], v_param=[0, 1], predict_x0=[0, 1], update=["none", "first", "second"], want_m=[0, 1], n=[420])
                             + [dict(branches=2, v_param=1, predict_x0=1, update="second", want_m=1, n=_W, wrap=True)]),
    "ae_silu_to_bf16": [dict(in_bf16=0, n=257), dict(in_bf16=1, n=257), dict(in_bf16=0, n=_W, wrap=True)],
    "ae_add_bcast_bf16": _prod(period=[8, 320], reps=[1, 3]) + [dict(period=8, reps=_W, wrap=True)],
    "ae_resample2x_rows_bf16": [dict(B=2, H=3, W=5, C=8, down=0), dict(B=2, H=5, W=7, C=16, down=1), dict(B=1, H=2, W=2, C=8, down=1),
                                dict(B=1, H=1, W=(_W + 3) // 4, C=8, down=0, wrap=True), dict(B=1, H=2, W=2 * _W, C=8, down=1, wrap=True)],
    "ae_scale_shift_rows_bf16": [dict(B=3, HW=5, C=16, silu=0), dict(B=3, HW=5, C=16, silu=1), dict(B=3, HW=_W // 3, C=8, silu=1, wrap=True)],
    "ae_window_partition_bf16": _WINDOW,
    "ae_sam_relpos_terms": _RELPOS,
    "ae_softmax_rows_f32_bf16": _prod(cols=[1, 63, 256, 257, 4100], scale=[1.0, 0.044194173824159216]),
    "ae_gaussian_moments_f32": _prod(noise=[0, 1], want_stats=[0, 1], B=[3], per=[35]) + [dict(noise=1, want_stats=1, B=3, per=_W // 3, wrap=True)],
    "ae_patchify_f32_bf16": [dict(B=2, Cin=3, H=28, W=42, P=14), dict(B=1, Cin=1, H=4, W=4, P=1), dict(B=2, Cin=3, H=32, W=16, P=16),
                             dict(B=3, Cin=3, H=1, W=_W // 9, P=1, wrap=True)],
    "ae_lincomb4_f32": _prod(terms=[1, 2, 3, 4], n=[1, 3, 4, 1023, 1024, 1025, 4099]),
    "ae_dpm_adaptive_err_f32": [dict(B=3, n=n, atol=0.0078, rtol=0.05, seed=30 + i) for i, n in enumerate((1, 63, 1024, 1025, 5000))],
    "ae_mse_f32": [dict(n=n) for n in (1, 257, 4100)] + [dict(n=MSE_WRAP, wrap=True), dict(n=_W, wrap=True)],
    # ---- backward.hip
    "ae_add_bf16": [dict(n=8), dict(n=2056), dict(n=8 * _W, wrap=True)],
    "ae_axpy_bf16": _prod(alpha=[0.0, 1.0, -0.5, 2.75], n=[8, 2056]) + [dict(alpha=-0.5, n=8 * _W, wrap=True)],
    "ae_geglu_fwd_bf16": [dict(M=1, F=8), dict(M=5, F=1280), dict(M=37, F=24), dict(M=_W, F=8, wrap=True)],
    "ae_geglu_bwd_bf16": [dict(M=1, F=8), dict(M=5, F=1280), dict(M=37, F=24), dict(M=_W, F=8, wrap=True)],
    "ae_sumpool2x2_bf16": [dict(B=2, H=3, W=5, C=8), dict(B=1, H=1, W=1, C=16), dict(B=1, H=1, W=_W, C=8, wrap=True)],
    "ae_colsum_bf16_f32": [dict(M=1, N=1, ld=1), dict(M=1000, N=255, ld=255), dict(M=7, N=256, ld=256), dict(M=7, N=257, ld=257), dict(M=7, N=257, ld=264)],
    "ae_mse_grad_f32": _prod(n=[1, 257, 4100], loss_scale=[1.0, 128.0]) + [dict(n=_W, loss_scale=128.0, wrap=True)],
    "ae_adamw_f32": _prod(start=[1, 1000], weight_decay=[0.0, 1e-2], grad_scale=[1.0, 1.0 / 128], n=[1025]) + [dict(start=1, weight_decay=1e-2, grad_scale=1.0, n=_W, wrap=True)],
    "ae_scatter_add_rows_f32": _prod(D=[1, 255, 768], code_dtype=["i32", "i64"]),
    "ae_rowsum_f32": [dict(rows=3, n=5000), dict(rows=4, n=32768), dict(rows=4, n=4100), dict(rows=4, n=1027), dict(rows=4, n=3), dict(rows=3, n=1029)],
    # ---- gate.hip
    "ae_task_gate": _GATE_FWD,
    "ae_task_gate_bwd": _GATE_BWD,
    "ae_task_gate_wgrad": _GATE_BWD,
    # ---- expert_kv.hip
    "ae_expert_kv_fwd": _EXPERT,
    "ae_expert_kv_dgrad": _EXPERT,
    "ae_expert_kv_wgrad": _EXPERT,
}
SOURCES = ("elementwise.hip", "backward.hip", "gate.hip", "expert_kv.hip")
NOT_A_LAUNCH = {"ae_expert_kv_dgrad_slices"}      # returns a size; nothing to compare
