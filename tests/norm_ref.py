"""Seeded operands, float64 references and element-wise bounds of the GroupNorm / LayerNorm route cases (tests/route_cases.py, NORM_CASES),
shared by tools/norm_route_check.py (GPU) and tests/test_norm_ref.py (CPU: the bounds must reject five kinds of wrong kernel).

Everything is written for GroupNorm on [B, HW, C] with `groups`; LayerNorm over [M, C] is the same thing with B = M, HW = 1, groups = 1.

Data.  x[b, :, g] = mu_bg + sigma_bg * randn, rounded to bf16; sigma_bg uniform in [0.5, 2], mu_bg / sigma_bg drawn from
{0, +-0.25, +-4, +-16}: every (sample, group) has statistics of its own, so a wrong group or sample index moves the answer by far more than
the bound.  One (sample, group) of every GroupNorm case is constant (sigma = 0).  gamma / beta: random, about a sixth exact zeros, half of
gamma negative.

Bounds.  a = 2^-16 is the project's fp32 accumulation constant (256 unit roundoffs: above the random walk of every sum here, far below one
bf16 rounding, 2^-8).  With r = rstd, rho = |mu| r:
  statistics (a route that delivers them):   two-pass (mean, then centred squares: slab kernels, every LayerNorm)   e_r = a
                                             one-pass (E[x^2] - mean^2 in fp32: three launches, producer statistics)  e_r = a (1 + rho^2) / 2
        |rstd^ / rstd - 1| <= e_r            (var = E[x^2] - mean^2 carries the fp32 error of E[x^2] = sigma^2 (1 + rho^2); rstd half of it)
        |mean^ - mean| r  <= e_mu = a (1 + rho)     (the fp32 error of a sum of terms of size sigma + |mu|, in units of sigma)
  forward, every element:   y = act(xhat gamma + beta)
        |got - ref| <= 2^-8 |ref| + s ( |gamma| (|xhat| e_r + e_mu) + a (|gamma| r (|x| + |mu|) + |beta|) )
     one bf16 rounding of the result; the statistics' allowances carried through xhat = (x - mean) r; a times the absolute terms of
     x r gamma - mean r gamma + beta as the kernels evaluate it (x * scale + shift); s = the activation's largest slope (SiLU 1.1, GELU 1.13).
  backward, every element:  t = dy act'(z) gamma,  m1 = mean_g(t),  m2 = mean_g(t xhat),  dx = r (t - m1 - xhat m2)  (+ old under accumulate)
     with X = r (|x| + |mu|) (the absolute terms of xhat), d = |xhat| e_r + e_mu (its statistics allowance), dt = |gamma| |dy| c2 (|gamma| d +
     a (|gamma| X + |beta|)) (the error of t through act'(z): c2 = max |act''| = 0.5 for SiLU, 0 without activation):
        |got - ref| <= (1 + acc) 2^-8 |ref| + a |old|                                     one bf16 rounding, two under accumulate
                       + a r (|t| + mean|t| + X mean(|t| X))                               fp32 evaluation of the expression and of its two means
                                                                                           (the three-launch form x kA + kB cancels at the size of X)
                       + e_r r (|t| + mean|t| + |xhat| mean|t xhat|)                       the factor r
                       + r (dt + mean(dt) + |xhat| mean(dt |xhat| + |t| d) + d mean|t xhat|)   xhat and t inside the expression and the means
     parameter gradients (fp32, M <= 4096 rows): dgamma = sum_m dy xhat, dbeta = sum_m dy:
        |got - ref| <= 2^-20 |ref| + a sum|dy xhat| + sum |dy| d     resp.    2^-20 |ref| + a sum|dy|.
"""
import torch

BF = torch.bfloat16
F64 = torch.float64
A_ACC = 2.0 ** -16
RATIOS = (0.0, 0.25, -0.25, 4.0, -4.0, 16.0, -16.0)
SLOPE = {0: 1.0, 1: 1.1, 2: 1.13}      # act: 0 none, 1 SiLU, 2 GELU
CURV = {0: 0.0, 1: 0.5}                # max |act''|


class BoundFailure(Exception):
    pass


# --------------------------------------------------------------------------------------------------- operands
def make_x(gen, B, HW, C, groups, ratio=None, const_group=True):
    """bf16 [B, HW, C] with per-(sample, group) mean and spread; ratio: a fixed |mu / sigma| for every group (the conditioning sweep)"""
    cpg = C // groups
    sigma = 0.5 + 1.5 * torch.rand(B, groups, generator=gen, dtype=F64)
    if ratio is None:
        rat = torch.tensor(RATIOS, dtype=F64)[torch.randint(0, len(RATIOS), (B, groups), generator=gen)]
    else:
        rat = ratio * (2.0 * torch.randint(0, 2, (B, groups), generator=gen).to(F64) - 1.0)
    mu = rat * sigma
    if const_group:
        b, g = int(torch.randint(0, B, (1,), generator=gen)), int(torch.randint(0, groups, (1,), generator=gen))
        sigma[b, g], mu[b, g] = 0.0, -1.25
    z = torch.randn(B, HW, groups, cpg, generator=gen, dtype=F64)
    x = mu[:, None, :, None] + sigma[:, None, :, None] * z
    return x.reshape(B, HW, C).to(BF)


def make_affine(gen, C):
    gamma = torch.randn(C, generator=gen) * 0.5 + torch.where(torch.rand(C, generator=gen) < 0.5, 1.0, -1.0)
    beta = torch.randn(C, generator=gen) * 0.5
    gamma[torch.rand(C, generator=gen) < 1 / 6] = 0.0
    beta[torch.rand(C, generator=gen) < 1 / 6] = 0.0
    return gamma.float(), beta.float()


def slab_sums(x, rows=32):
    """the producers' column statistics of x [M, C] bf16: float64 (sum, sum of squares) per 32-row slab and channel, rounded to fp32"""
    M, C = x.shape
    xs = x.to(F64).reshape(M // rows, rows, C)
    return torch.stack([xs.sum(1), (xs * xs).sum(1)], -1).float().contiguous()


# --------------------------------------------------------------------------------------------------- reference
def _act(z, act):
    if act == 1:
        return z * torch.sigmoid(z)
    if act == 2:
        return 0.5 * z * (1.0 + torch.erf(z / 2 ** 0.5))
    return z


def _act_grad(z, act):
    if act == 1:
        sg = torch.sigmoid(z)
        return sg * (1.0 + z * (1.0 - sg))
    return torch.ones_like(z)


def _per_channel(t, cpg):
    """[B, groups] -> [B, 1, C]"""
    return t.repeat_interleave(cpg, 1)[:, None, :]


def _group_mean(t, groups):
    """mean over (HW, channels of the group) of t [B, HW, C], spread back to [B, 1, C]"""
    B, HW, C = t.shape
    return _per_channel(t.reshape(B, HW, groups, C // groups).mean((1, 3)), C // groups)


def statistics(x, groups, eps):
    """float64 (mean, rstd) [B, groups] of x [B, HW, C]"""
    B, HW, C = x.shape
    xg = x.to(F64).reshape(B, HW, groups, C // groups)
    m = xg.mean((1, 3))
    v = ((xg - m[:, None, :, None]) ** 2).mean((1, 3))
    return m, (v + eps).rsqrt()


def allowances(mean, rstd, onepass):
    rho = mean.abs() * rstd
    e_r = A_ACC * (1.0 + rho * rho) / 2.0 if onepass else torch.full_like(rho, A_ACC)
    return e_r, A_ACC * (1.0 + rho)


def forward(x, gamma, beta, groups, eps, act, onepass, mean=None, rstd=None):
    """-> dict(mean, rstd [B, groups]; xhat, z, y, bnd [B, HW, C]).  mean / rstd: statistics to normalise with (tests of the bound feed
    wrong ones); the bound always belongs to the true ones."""
    x = x.to(F64)
    B, HW, C = x.shape
    cpg = C // groups
    m0, r0 = statistics(x, groups, eps)
    m, r = (m0 if mean is None else mean), (r0 if rstd is None else rstd)
    g, bt = gamma.to(F64), beta.to(F64)
    xhat = (x - _per_channel(m, cpg)) * _per_channel(r, cpg)
    z = xhat * g + bt
    y = _act(z, act)
    e_r, e_mu = allowances(m0, r0, onepass)
    R, MU = _per_channel(r0, cpg), _per_channel(m0, cpg)
    bnd = 2.0 ** -8 * y.abs() + SLOPE[act] * (g.abs() * (xhat.abs() * _per_channel(e_r, cpg) + _per_channel(e_mu, cpg))
                                              + A_ACC * (g.abs() * R * (x.abs() + MU.abs()) + bt.abs())) + 1e-30
    return dict(mean=m0, rstd=r0, xhat=xhat, z=z, y=y, bnd=bnd)


def backward(x, gamma, beta, dy, groups, eps, act, onepass, old=None, acc_mask=None):
    """-> dict(dx, bnd [B, HW, C]; dgamma, dbeta, bnd_dgamma, bnd_dbeta [C] (sums over B and HW: LayerNorm's parameter gradients)).
    old: the gradient already in the target ([B, HW, C]); acc_mask: [C] 1.0 where the kernel adds to it (default: everywhere)"""
    x, dy = x.to(F64), dy.to(F64)
    B, HW, C = x.shape
    cpg = C // groups
    f = forward(x, gamma, beta, groups, eps, act, onepass)
    g, bt = gamma.to(F64), beta.to(F64)
    xhat, z = f["xhat"], f["z"]
    R, MU = _per_channel(f["rstd"], cpg), _per_channel(f["mean"], cpg)
    e_r, e_mu = allowances(f["mean"], f["rstd"], onepass)
    ER, EM = _per_channel(e_r, cpg), _per_channel(e_mu, cpg)
    t = dy * _act_grad(z, act) * g
    gm = lambda v: _group_mean(v, groups)   # noqa: E731
    dx = R * (t - gm(t) - xhat * gm(t * xhat))
    ref = dx if old is None else dx + old.to(F64)
    X = R * (x.abs() + MU.abs())
    d = xhat.abs() * ER + EM
    dt = g.abs() * dy.abs() * CURV[act] * (g.abs() * d + A_ACC * (g.abs() * X + bt.abs()))
    ta, xa = t.abs(), xhat.abs()
    nround = 1.0 if old is None else 1.0 + (torch.ones(C, dtype=F64) if acc_mask is None else acc_mask.to(F64))
    bnd = (nround * 2.0 ** -8 * ref.abs() + (A_ACC * old.to(F64).abs() if old is not None else 0.0)
           + A_ACC * R * (ta + gm(ta) + X * gm(ta * X))
           + ER * R * (ta + gm(ta) + xa * gm(ta * xa))
           + R * (dt + gm(dt) + xa * gm(dt * xa + ta * d) + d * gm(ta * xa)) + 1e-30)
    dxh = dy * xhat
    out = dict(dx=ref, bnd=bnd, dgamma=dxh.sum((0, 1)), dbeta=dy.sum((0, 1)))
    out["bnd_dgamma"] = 2.0 ** -20 * out["dgamma"].abs() + A_ACC * dxh.abs().sum((0, 1)) + (dy.abs() * d).sum((0, 1)) + 1e-30
    out["bnd_dbeta"] = 2.0 ** -20 * out["dbeta"].abs() + A_ACC * dy.abs().sum((0, 1)) + 1e-30
    return out


# --------------------------------------------------------------------------------------------------- window partition (SAM)
def window_rows(B, H, W, ws):
    """-> (img [rows] long: image row of every window row, -1 for a padding row)"""
    nH, nW = (H + ws - 1) // ws, (W + ws - 1) // ws
    b, jh, jw, wy, wx = torch.meshgrid(torch.arange(B), torch.arange(nH), torch.arange(nW), torch.arange(ws), torch.arange(ws), indexing="ij")
    yy, xx = jh * ws + wy, jw * ws + wx
    img = (b * H + yy) * W + xx
    img[(yy >= H) | (xx >= W)] = -1
    return img.reshape(-1)


# --------------------------------------------------------------------------------------------------- checks
def check_elements(got, ref, bnd, what):
    """every element of `got` within `bnd` of `ref`; returns the worst error / bound"""
    got = got.to(F64)
    if got.shape != ref.shape:
        raise BoundFailure(f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}")
    if not torch.isfinite(got).all():
        raise BoundFailure(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values")
    q = (got - ref).abs() / bnd
    ratio = float(q.max())
    if ratio > 1.0:
        i = int(q.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise BoundFailure(f"{what}: element {idx} got {float(got.flatten()[i]):.6g} ref {float(ref.flatten()[i]):.6g} bound "
                           f"{float(bnd.flatten()[i]):.3g} (ratio {ratio:.2f}); {int((q > 1).sum())} of {q.numel()} elements fail")
    return ratio


def check_statistics(stat, mean, rstd, onepass, what="statistics"):
    """stat [B, groups, 2] (mean, rstd) from the kernel; returns the worst error / allowance"""
    stat = stat.to(F64)
    if not torch.isfinite(stat).all():
        raise BoundFailure(f"{what}: non-finite values")
    e_r, e_mu = allowances(mean, rstd, onepass)
    q_r = (stat[..., 1] / rstd - 1.0).abs() / e_r
    q_m = (stat[..., 0] - mean).abs() * rstd / e_mu
    ratio = float(torch.maximum(q_r, q_m).max())
    if ratio > 1.0:
        i = int(torch.maximum(q_r, q_m).flatten().argmax())
        b, g = divmod(i, mean.shape[1])
        raise BoundFailure(f"{what}: (sample {b}, group {g}) mean {float(stat[b, g, 0]):.8g} ref {float(mean[b, g]):.8g}, rstd {float(stat[b, g, 1]):.8g} "
                           f"ref {float(rstd[b, g]):.8g}: rstd error / allowance {float(q_r[b, g]):.2f}, mean error / allowance {float(q_m[b, g]):.2f}")
    return ratio


def check_pad_rows(got, pad):
    """rows of the window partition's padding (pad: bool [rows]) must be exactly +0"""
    bits = got.contiguous().view(torch.int16)[pad]
    if bool((bits != 0).any()):
        raise BoundFailure(f"padding rows: {int((bits != 0).sum())} elements are not zero")
