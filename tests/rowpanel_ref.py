"""Seeded operands, float64 references and element-wise bounds of the row-panel GEMM / fused feed-forward route cases (tests/route_cases.py,
ROWPANEL_CASES), shared by tools/rowpanel_route_check.py (GPU) and tests/test_rowpanel_ref.py (CPU: the bounds must reject fourteen kinds of
wrong kernel).  `bound_check`, `stats_check` and the constant a = 2^-16 are those of tools/route_check.py.

Data.  Activation rows: 1.3 randn + a row mean of 1.3 clamp(randn, -2, 2) (up to two standard deviations, the case a LayerNorm's subtraction has
to survive), rounded to bf16; every 37th row instead 2^-7 randn with no mean — a variance of 6e-5, where eps = 1e-5 inside or outside the root
differs by 5 % in rstd.  Weights randn / sqrt(K), biases 0.1 randn, gamma = 1 + 0.2 randn, beta = 0.2 randn.  (The row mean of
test_feed_forward_fused_one_launch, 2 randn = up to 4.6 standard deviations, makes 10.4 % of the LayerNorm operands ambiguous in the sense below —
the allowance grows with rho — which is past the 10 % cap; with the means used here it is about 8 %.)

Bounds, every element (a = 2^-16; 2^-8 |ref| is the one bf16 rounding of the stored output):
  plain GEMM          |got - ref| <= 2^-8 |ref| + a (|A| |W| + |bias| + |res|)
  GEGLU               ref = ya gelu(yg) on the chunk(2) halves of the pre-activation y = A W^T + b; with the pre-activation allowances da, dg
                      (a (|A| |W| + |b|) of either half):  2^-8 |ref| + |gelu(yg)| da + 1.13 |ya| dg + 1.13 da dg     (|gelu'| <= 1.13)
  LayerNorm fold      y = rstd (x W'^T - mean s) + c from the float64 statistics of the stored bf16 x and (W', s, c) of ops.pack_ln_fold:
                      the allowance of the pre-activation is a (rstd (|x| |W'| + |mean| |s|) + |c|)  (+ a |res|)
  LayerNorm prologue  the kernel rounds z = xhat gamma + beta to bf16 for the MFMA; the reference rounds the float64 z the same way.  The
                      fp32 z of a correct two-pass LayerNorm lies within  al = |gamma| (|xhat| a + a (1 + rho)) + a (|gamma| rstd (|x| + |mean|)
                      + |beta|)  of it (tests/norm_ref.py: statistics allowances e_r = a, e_mu = a (1 + rho), rho = |mean| rstd, and the fp32
                      affine term), so its rounding lies between round(z - al) and round(z + al):  dev = max(round(z + al) - round(z),
                      round(z) - round(z - al)), zero unless a rounding boundary lies within al of z (the element is then AMBIGUOUS and
                      dev is one bf16 ulp of z; two where al spans two boundaries).  The pre-activation allowance gains sum_k dev_k |W_nk|.
                      The share of ambiguous operand elements of a case must stay <= 10 % (asserted on the CPU from the reference alone).
  feed-forward        through the STORED hidden activation h_s = ops.ln_gemm(..., EPI_GEGLU) (itself checked by the prologue rule; the fused
                      kernel's gated values are bit-identical to that epilogue, ff_fused.hip's header):
                      |y - ref'| <= 2^-8 |ref'| + a (|h_s| |W2| + |b2| + |R|),  ref' = float64(h_s W2^T + b2 + R);
                      with the projection: z against float64(y_s W3^T + b3 + R3), y_s the stored output without it, same rule.
                      MEASURED (MI355X): that header's claim does not hold — about one LayerNorm operand in 10^5 is rounded to the other
                      bf16 neighbour by the two kernels' separately compiled prologues, and several of that row's hidden values then
                      differ by an ulp (459 of 2.3 million at M = 36673, H = 64, in 95 rows; both kernels within the prologue rule).  So
                      a. against h_s the bound gains  sum_h dev_h |W2_nh|,  dev_h = round(ref_h + d_h) - round(ref_h - d_h) with d_h the
                         prologue rule's allowance of the float64 hidden value ref_h in front of its rounding (`hidden_deviation`: the two
                         stored values of a hidden unit both lie in that interval).  98 % of the hidden values are ambiguous in this sense
                         and the bound is 12 (H = 64) to 50 (H = 1280) output roundings wide: it still rejects a skipped chunk, a missing
                         b2 and a W2 image read without its rotation (9 to 270 times over), but no longer a single wrong term;
                      b. the tight rule is therefore applied to the fused kernel's OWN hidden activation h_f — W2 := a 0/1 selection of 320
                         hidden units, b2 = 0, no residual makes the kernel store h_f exactly — which is itself checked against the
                         prologue rule element by element, and y against float64(h_f W2^T + b2 + R) with the bound as first stated.
  statistics          `stats_check` on the stored bf16 output: |got - sum| <= a sum|y|, |got - sum y^2| <= a sum y^2.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

from route_check import A_ACC, CaseFailure, bound_check, gelu64, stats_check  # noqa: E402,F401

BF = torch.bfloat16
F64 = torch.float64
K = 320
SLOPE = 1.13
AMBIGUOUS_CAP = 0.10
SMALL_EVERY = 37


# --------------------------------------------------------------------------------------------------- operands
def make_rows(gen, M, C=K):
    x = torch.randn(M, C, generator=gen) * 1.3 + torch.randn(M, 1, generator=gen).clamp(-2.0, 2.0) * 1.3
    small = torch.arange(SMALL_EVERY - 1, M, SMALL_EVERY)
    x[small] = torch.randn(len(small), C, generator=gen) * 2.0 ** -7
    return x.to(BF)


def make_weight(gen, N, Kin):
    """fp32 master weight [N, Kin]"""
    return torch.randn(N, Kin, generator=gen) / Kin ** 0.5


def make_bias(gen, N):
    return 0.1 * torch.randn(N, generator=gen)


def make_affine(gen, C=K):
    return 1.0 + 0.2 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)


# --------------------------------------------------------------------------------------------------- bf16 grid in float64
def round_bf16(v):
    """round-to-nearest-even of float64 values to the bf16 grid (8 significant bits), kept in float64"""
    m, e = torch.frexp(v)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def ulp_bf16(v):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 8)


# --------------------------------------------------------------------------------------------------- references
def row_statistics(x, eps):
    x = x.to(F64)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return mu, (var + eps).rsqrt()


def ln_prologue(x, gamma, beta, eps):
    """-> dict(zb: the MFMA operand [M, K] (float64 values on the bf16 grid), dev: how far a correct kernel's operand may sit from it, share:
    the fraction of ambiguous elements)"""
    x = x.to(F64)
    mu, r = row_statistics(x, eps)
    g, b = gamma.to(F64), beta.to(F64)
    xhat = (x - mu) * r
    z = xhat * g + b
    rho = mu.abs() * r
    al = g.abs() * (xhat.abs() * A_ACC + A_ACC * (1.0 + rho)) + A_ACC * (g.abs() * r * (x.abs() + mu.abs()) + b.abs())
    zb = round_bf16(z)
    dev = torch.maximum(round_bf16(z + al) - zb, zb - round_bf16(z - al))
    return dict(z=z, zb=zb, dev=dev, al=al, share=float((dev > 0).to(F64).mean()))


def _finish(pre, P, E, res, geglu, packed):
    """pre-activation `pre`, its absolute terms P (enter with a) and its operand allowance E (enters as it is) -> (ref, bound)"""
    d = A_ACC * P + E
    if geglu:
        if packed:       # rows interleaved 16 a / 16 gate (the kernel's own layout)
            M, N = pre.shape
            ya, yg = pre.reshape(M, N // 32, 2, 16).unbind(2)
            da, dg = d.reshape(M, N // 32, 2, 16).unbind(2)
            ya, yg, da, dg = (t.reshape(M, N // 2) for t in (ya, yg, da, dg))
        else:            # attention.py GEGLU: x, gate = proj(x).chunk(2, dim=-1)
            (ya, yg), (da, dg) = pre.chunk(2, 1), d.chunk(2, 1)
        gl = gelu64(yg)
        ref, acc = ya * gl, gl.abs() * da + SLOPE * ya.abs() * dg + SLOPE * da * dg
    else:
        ref, acc = pre, d
    if res is not None:
        res = res.to(F64)
        ref, acc = ref + res, acc + A_ACC * res.abs()
    return ref, 2.0 ** -8 * ref.abs() + acc + 1e-30


def gemm_ref(A, W, bias=None, res=None, geglu=False, dev=None):
    """A [M, K]: the operand as the MFMA sees it; W [N, K]: bf16 weight in the ORIGINAL row order ([a rows | gate rows] for GEGLU);
    dev [M, K]: allowance of the operand itself (LayerNorm prologue)"""
    A, W = A.to(F64), W.to(F64)
    pre, P = A @ W.t(), A.abs() @ W.abs().t()
    if bias is not None:
        pre, P = pre + bias.to(F64), P + bias.to(F64).abs()
    E = dev @ W.abs().t() if dev is not None else torch.zeros_like(pre)
    return _finish(pre, P, E, res, geglu, False)


def ln_gemm_ref(x, gamma, beta, eps, W, bias=None, res=None, geglu=False):
    p = ln_prologue(x, gamma, beta, eps)
    ref, bnd = gemm_ref(p["zb"], W, bias, res, geglu, dev=p["dev"])
    return ref, bnd, p["share"]


def hidden_deviation(ref_h, bnd_h):
    """how far apart two kernels that both satisfy the prologue rule may STORE a hidden value: each one's fp32 value lies within
    d = bnd_h - 2^-8 |ref_h| of the float64 ref_h, so its bf16 rounding lies in [round(ref_h - d), round(ref_h + d)]"""
    d = bnd_h - 2.0 ** -8 * ref_h.abs()
    return round_bf16(ref_h + d) - round_bf16(ref_h - d)


def pack_ln_fold_ref(w, bias, gamma, beta, geglu, pack_geglu):
    """the definition of ops.pack_ln_fold on the CPU: W' = bf16(W gamma) (fp32 product), s = row sums of W', c = W beta + b"""
    wf = w.float()
    c = (wf.to(F64) @ beta.to(F64) + bias.to(F64)).float()
    wp = wf * gamma.float()[None, :]
    if geglu:
        wq, c = pack_geglu(wp, c)
    else:
        wq = wp.to(BF)
    return wq, wq.to(F64).sum(1).float(), c


def fold_ref(x, wq, s, c, eps, res=None, geglu=False):
    """x: the stored bf16 rows; (wq, s, c): pack_ln_fold's, in the packed row order"""
    x, W, s, c = x.to(F64), wq.to(F64), s.to(F64), c.to(F64)
    mu, r = row_statistics(x, eps)
    pre = r * (x @ W.t() - mu * s) + c
    P = r * (x.abs() @ W.abs().t() + mu.abs() * s.abs()) + c.abs()
    return _finish(pre, P, torch.zeros_like(pre), res, geglu, True)


def check(got, ref, bnd, what):
    """every element; returns the worst error / bound, raises CaseFailure beyond 1"""
    if tuple(got.shape) != tuple(ref.shape):
        raise CaseFailure(f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}")
    return bound_check(got.float(), ref, bnd, what)


def row_stats_check(got, y, what="row statistics"):
    """got fp32 [M, N / 64, 2] against the stored bf16 y [M, N]"""
    return stats_check(got, y.float(), 64, what, per_row=True)
