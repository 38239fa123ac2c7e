"""Seeded operands, float64 references and element-wise bounds of the coordinate, box and mask kernels (csrc/msda.hip, sam_decoder.hip),
shared by tests/test_hip_geom_kernels.py (GPU) and tests/test_geom_ref.py (CPU: the references against the oracle and torch's own operators,
the bounds against deliberately wrong results).  torch on the CPU only; nothing here imports the extension or the oracle.

Every reference is written from the formula in the kernel's header comment, in float64 over the exact fp32 / bf16 input values.  CASES
names, per `extern "C"` entry point of the two sources, the cases the GPU file runs.  `wrong=` of msda_eval / the `variant=` arguments
select the wrong kernels of tests/test_geom_ref.py; the references never pass them.

Bound families.  They extend the list of tests/small_ref.py ((a)-(f)); a = 2^-16, 2^-8 = one bf16 rounding, u = 2^-24 = fp32 unit roundoff.
  (g) fp32 sum of K products (ae_linear_f32)        |got - ref| <= (K + 2) u (sum_k |x w| + |b|)
                     the running-error bound of a K-term fma chain plus the bias add: what "exact fp32" means.
  (d) kernel-ordered fp32 sums                      |got - ref| <= a sum|terms| + 2^-20 |ref|     (small_ref's family (d))
                     mask product; MSDA grad_value (float atomics); grad_weight / grad_loc on the atomic path (d/4 not a power of two).
  (h) gather at an fp32 coordinate                  |got - ref| <= n u sum|terms| + sum_axes e_c |slope|
                     n counts the roundings on the longest path of one term, e_c is the fp32 error of the pixel coordinate (or phase) and
                     the slope is taken from the reference's own corners.
       MSDA:  x = loc W - 0.5 is two roundings (the product, the subtraction; one if the compiler fuses them) and lx = x - floor(x) a third
              (inexact only for x in (-1, 0)):  e_c = u (|loc W| + |x| + 1), three half-ulps of at most the coordinate's own size.
              forward      n = L P + 10  (three for a corner weight, one product, four corner adds, the weight, L P sample adds, one spare);
                           slope = d bilinear / dx, dy per channel  (= the location gradient of one channel divided by W, H)
              grad_weight  n = d + 10 on the shuffle path (a d-term dot, the corner weights), family (d)'s first two terms on the atomic
                           path; slope = grad_loc / (weight W), grad_loc / (weight H)
              grad_loc     the same n;  grad_loc.x depends on y alone inside a cell: slope = |w| W (|d00| + |d01| + |d10| + |d11|)
              grad_value   family (d) plus (e_cx + e_cy) |w g| at every corner a sample touches (a corner weight has slope <= 1)
              Cell boundaries.  Where the float64 coordinate lies within e_c of an integer the kernel may floor into either neighbour.  The
              sampled value and grad_weight are continuous there, so their bound is the larger of the two cells'; grad_loc is not, and has
              to lie within the bound of the reference of ONE of the two cells (four with both axes).  On a power-of-two level the fp32
              coordinate of loc = (k + 0.5) / W is exactly k (every operation is exact): no choice is allowed there — floor selects the
              cell, lx = 0, the gradient is the right / lower cell's, a far corner outside the level reads 0.
              Outside (x <= -1, x >= W, y <= -1, y >= H): no term and no slope, the bound collapses to 1e-30: exactly 0.
       pe_encode:  the phase 2 pi ((2x - 1) g0 + (2y - 1) g1) takes eight roundings (c + offset, the product with 1/W and 1/W's own
              rounding, 2x - 1, the product with g, the sum, the product with 2 pi and 2 pi's own rounding), each of at most the phase's
              absolute terms P = 2 pi ((2|x| + 1)|g0| + (2|y| + 1)|g1|); sin and cos have slope <= 1 and are returned to 2 ulp; the label
              row is one more add:  |got - ref| <= u (8 P + 4 (|enc| + |row|));  label -1 writes the row itself: exact.
       postprocess:  the source coordinate scale (dst + 0.5) - 0.5 is three roundings (the fp32 scale, the product, the subtraction):
              e_c = u (2 scale (dst + 0.5) + |s|); each bilinear stage is "a few fp32 operations" (family (b)'s 2^-22) on its sum|terms|;
              the slope is the largest of the cell's and its two neighbours' differences (a coordinate within e_c of an integer may
              floor either way; the interpolant is continuous); stage one's allowance is interpolated by stage two's (non-negative)
              weights.
  (i) bf16 result after two LayerNorms over 4 and 16 channels (ae_sam_mask_downscale_bf16)
                     tests/norm_ref.py's two-pass LayerNorm allowances (e_r = a, e_mu = a (1 + rho)) and absolute terms, carried through
                     both stages: with dt the error of a LayerNorm's input (max over its channels), xhat moves by at most
                     r (2 + |xhat|) dt (the mean moves it by dt, rstd by r dt |xhat|);
                       dt1 = 2^-22 (|b1| + sum|w1 m|)                                            (family (b), fp32)
                       Ez  = |g| (|xhat| e_r + e_mu + r (2 + |xhat|) dt) + a (|g| r (|t| + |mu|) + |e|)
                       dt2 = sum |w2| 1.13 Ez1 + a (|b2| + sum |w2 gelu(z1)|)                    (family (d) through the second convolution)
                       |got - ref| <= 2^-8 |ref| + 1.13 Ez2
  (j) decided        preprocess' padding is +0.0 by bits and its pixels are family (b) in fp32 (2^-22 (|x| + |mean|) / |std|); the binary
                     mask of postprocess equals (ref > threshold) wherever |ref - threshold| exceeds the logit's bound (h), the merged
                     union wherever one mask is decidedly above or all are decidedly below; nms keep flags equal the float64 greedy pass
                     (test_geom_ref.py asserts that no IoU of a random case lies within 2^-20 relative of the threshold: an fp32 IoU is
                     ten roundings; the built cases are exact in fp32).
"""
import math
import types

import torch

from small_ref import BF_EPS, TINY, A, BoundFailure, _prod, bound_d, c32, check_bits, check_elements, gelu64, gen, randn  # noqa: F401

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
SLOPE_GELU = 1.13
PRODUCT_WRAP = (257, 256)        # (h, w): 16 h w = 1 052 672 pixels against one pass of 4096 blocks x 256 threads


def pow2(n):
    return n > 0 and (n & (n - 1)) == 0


def check_any(got, refs, bnds, what):
    """every element of `got` within the bound of at least one of the references; returns the worst (best-of) error / bound"""
    got = got.to(F64)
    if not torch.isfinite(got).all():
        raise BoundFailure(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values")
    q = torch.stack([(got - r).abs() / b for r, b in zip(refs, bnds)]).min(0).values
    ratio = float(q.max()) if q.numel() else 0.0
    if ratio > 1.0:
        i = int(q.flatten().argmax())
        raise BoundFailure(f"{what}: flat element {i} got {float(got.flatten()[i]):.9g} ref {float(refs[0].flatten()[i]):.9g} bound "
                           f"{float(bnds[0].flatten()[i]):.3g} (ratio {ratio:.2f}); {int((q > 1).sum())} of {q.numel()} elements fail")
    return ratio


# =================================================================================================== (g) ae_linear_f32
def linear_case(c):
    g = gen(1000 + 7 * c["M"] + 3 * c["N"] + c["K"])
    x, w = randn(g, c["M"], c["K"]), randn(g, c["N"], c["K"], scale=1.0 / math.sqrt(c["K"]))
    b = randn(g, c["N"]) if c["bias"] else None
    return x, w, b


def ref_linear(x, w, b):
    ref = x.to(F64) @ w.to(F64).t()
    terms = x.to(F64).abs() @ w.to(F64).abs().t()
    if b is not None:
        ref, terms = ref + b.to(F64), terms + b.to(F64).abs()
    return ref, (x.shape[1] + 2) * U * terms + TINY


# =================================================================================================== (h) MSDA
MSDA_CLASSES = ("inside", "frame", "rim1", "rim2", "edge", "far", "centre")
MSDA_WRONG = ("swap_xy", "swap_wh", "align_corners", "clamp_rim", "drop_corner", "level_row", "no_wh", "gw_times_w")


def _place(name, r, j, H, W):
    """(loc_x, loc_y) float64 of class `name` for every sample; r [n, 4] uniform, j [n] a counter that alternates side and axis"""
    side, side2, axis = j % 2 == 1, (j // 2) % 2 == 1, (j // 4) % 2 == 1
    size = torch.where(axis, torch.tensor(float(H), dtype=F64), torch.tensor(float(W), dtype=F64))
    ins = [(r[:, 0] * (W - 1) + 0.5) / W, (r[:, 1] * (H - 1) + 0.5) / H]
    u = 0.05 + 0.9 * r[:, 2:4]
    rim = [(torch.where(s, n - 1.0 + u[:, i], -1.0 + u[:, i]) + 0.5) / n for i, (n, s) in enumerate(((W, side), (H, side2)))]

    def on_axis(special):      # `special` on the chosen axis, an inside coordinate on the other
        return torch.where(axis, ins[0], special), torch.where(axis, special, ins[1])
    if name == "inside":
        return ins[0], ins[1]
    if name == "frame":
        return on_axis(side.to(F64))
    if name == "rim1":
        return rim[0], rim[1]
    if name == "rim2":
        return torch.where(axis, ins[0], rim[0]), torch.where(axis, rim[1], ins[1])
    if name == "edge":         # exactly -1 px / size px where fp32 is exact (a power-of-two size), else pushed 2^-18 (>> e_c) further out
        at = (torch.where(side, size, torch.tensor(-1.0, dtype=F64)) + 0.5) / size
        exact = torch.where(axis, torch.tensor(pow2(H)), torch.tensor(pow2(W)))
        return on_axis(torch.where(exact, at, at * (1.0 + 2.0 ** -18)))
    if name == "far":
        return on_axis(torch.where(side, torch.tensor(4.0, dtype=F64), torch.tensor(-3.0, dtype=F64)))
    if name == "centre":
        return ((r[:, 0] * W).floor().clamp(max=W - 1) + 0.5) / W, ((r[:, 1] * H).floor().clamp(max=H - 1) + 0.5) / H
    raise KeyError(name)


def msda_case(c):
    """value, levels, locations by class (c['classes'] in turn, then one uniform in [-0.1, 1.1]; c['only']: the classes alone), weights with
    exact zeros and both signs, grad_out.  klass[b, q, h, l, p] = index into c['classes'] or -1."""
    g = gen(c["seed"])
    bs, Q, heads, d, P, levels = c["bs"], c["Q"], c["heads"], c["d"], c["P"], c["levels"]
    L, S = len(levels), sum(h * w for h, w in levels)
    cls = c["classes"]
    value, go = randn(g, bs, S, heads, d), randn(g, bs, Q, heads * d)
    w = randn(g, bs, Q, heads, L, P)
    w.view(-1)[::5] = 0.0
    loc = torch.empty(bs, Q, heads, L, P, 2, dtype=F64)
    klass = torch.empty(bs, Q, heads, L, P, dtype=torch.int64)
    n = bs * Q * heads * P
    per = len(cls) if c.get("only") else len(cls) + 1
    idx = torch.arange(n)
    k = idx % per
    k[k == len(cls)] = -1
    for l, (H, W) in enumerate(levels):
        r = torch.rand(n, 6, generator=g, dtype=F64)
        lx, ly = r[:, 4] * 1.2 - 0.1, r[:, 5] * 1.2 - 0.1
        for ci, name in enumerate(cls):
            px, py = _place(name, r, idx // per, H, W)
            lx, ly = torch.where(k == ci, px, lx), torch.where(k == ci, py, ly)
        loc[:, :, :, l, :, 0], loc[:, :, :, l, :, 1] = lx.reshape(bs, Q, heads, P), ly.reshape(bs, Q, heads, P)
        klass[:, :, :, l, :] = k.reshape(bs, Q, heads, P)
    shapes = torch.tensor(levels, dtype=torch.int64)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]])
    d4 = d // 4
    return types.SimpleNamespace(value=value, shapes=shapes, starts=starts, loc=loc.float(), weight=w, grad_out=go, klass=klass, c=c,
                                 dims=(bs, S, heads, d, Q, L, P), shuffle=pow2(d4) and d4 <= 64)


def msda_coords(cs, l):
    """float64 (x, y, e_cx, e_cy, near_x, near_y) of level l: pixel coordinates of the fp32 locations, their fp32 allowance, and whether an
    integer lies within it (never where fp32 is exact: a power-of-two size and an integer coordinate)"""
    H, W = (int(v) for v in cs.shapes[l])
    lx, ly = cs.loc[:, :, :, l, :, 0].to(F64), cs.loc[:, :, :, l, :, 1].to(F64)
    x, y = lx * W - 0.5, ly * H - 0.5
    ecx, ecy = U * ((lx * W).abs() + x.abs() + 1.0), U * ((ly * H).abs() + y.abs() + 1.0)
    nx = ((x - x.round()).abs() <= ecx) & ~((x == x.round()) & pow2(W))
    ny = ((y - y.round()).abs() <= ecy) & ~((y == y.round()) & pow2(H))
    return x, y, ecx, ecy, nx, ny


def msda_eval(cs, dtype=F64, wrong=None, alt=(0, 0)):
    """msda.hip's header formulas, forward and backward, in `dtype` (float64: the reference with its term magnitudes; float32: the correctly
    rounded result the bounds must accept).  alt = (1, .) / (., 1): samples within e_c of an integer column / row use the other adjacent cell."""
    bs, S, heads, d, Q, L, P = cs.dims
    v_all, w_all, loc = cs.value.to(dtype), cs.weight.to(dtype), cs.loc.to(dtype)
    go = cs.grad_out.to(dtype).reshape(bs, Q, heads, 1, d)
    want = dtype == F64 and wrong is None
    z = lambda *s: torch.zeros(*s, dtype=dtype)                                     # noqa: E731
    out, gv, gl, gw = z(bs, Q, heads, d), z(bs * S * heads, d), z(bs, Q, heads, L, P, 2), z(bs, Q, heads, L, P)
    T = types.SimpleNamespace(out=z(bs, Q, heads, d), c_out=z(bs, Q, heads, d), gv=z(bs * S * heads, d), c_gv=z(bs * S * heads, d),
                              gw=z(bs, Q, heads, L, P), c_gw=z(bs, Q, heads, L, P), gl=z(bs, Q, heads, L, P, 2), c_gl=z(bs, Q, heads, L, P, 2))
    outside = torch.zeros(bs, Q, heads, L, P, dtype=torch.bool)
    bi = torch.arange(bs).view(bs, 1, 1, 1).expand(bs, Q, heads, P)
    hi = torch.arange(heads).view(1, 1, heads, 1).expand(bs, Q, heads, P)
    for l in range(L):
        H, W = (int(v) for v in cs.shapes[l])
        s0 = int(cs.starts[l]) + (W if wrong == "level_row" else 0)
        lx_, ly_ = loc[:, :, :, l, :, 0], loc[:, :, :, l, :, 1]
        if wrong == "swap_xy":
            lx_, ly_ = ly_, lx_
        if wrong == "align_corners":
            x, y = lx_ * (W - 1), ly_ * (H - 1)
        elif wrong == "swap_wh":
            x, y = lx_ * H - 0.5, ly_ * W - 0.5
        else:
            x, y = lx_ * W - 0.5, ly_ * H - 0.5
        _, _, ecx, ecy, nx, ny = msda_coords(cs, l)
        ax, ay = (nx if alt[0] else torch.zeros_like(nx)), (ny if alt[1] else torch.zeros_like(ny))
        x0, y0, rx, ry = x.floor(), y.floor(), x.round(), y.round()
        x0, y0 = torch.where(ax, torch.where(x0 == rx, rx - 1, rx), x0), torch.where(ay, torch.where(y0 == ry, ry - 1, ry), y0)
        ins = (((x > -1) & (x < W)) | ax) & (((y > -1) & (y < H)) | ay)
        outside[:, :, :, l, :] = ~ins
        lx, ly = x - x0, y - y0
        cw = {(0, 0): (1 - ly) * (1 - lx), (0, 1): (1 - ly) * lx, (1, 0): ly * (1 - lx), (1, 1): ly * lx}
        if wrong == "drop_corner":
            del cw[(1, 1)]
        aw = w_all[:, :, :, l, :]
        t, dot, adot = {}, {}, {}
        for (dy, dx), wc in cw.items():
            yy, xx = (y0 + dy).long(), (x0 + dx).long()
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            if wrong == "clamp_rim":
                ok = torch.ones_like(ok)
            ok = ok & ins
            pix = (s0 + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)) % S
            t[(dy, dx)] = v_all[bi, pix, hi] * ok[..., None]                                  # [bs, Q, heads, P, d], zero outside
            rows = ((bi * S + pix) * heads + hi).reshape(-1)
            gv.index_add_(0, rows, ((aw * wc * ok)[..., None] * go).reshape(-1, d))
            if want:
                T.gv.index_add_(0, rows, ((aw * wc * ok).abs()[..., None] * go.abs()).reshape(-1, d))
                T.c_gv.index_add_(0, rows, (((ecx + ecy) * aw.abs() * ok)[..., None] * go.abs()).reshape(-1, d))
            dot[(dy, dx)], adot[(dy, dx)] = (t[(dy, dx)] * go).sum(-1), (t[(dy, dx)] * go).abs().sum(-1)
        if wrong == "drop_corner":
            t[(1, 1)], dot[(1, 1)], adot[(1, 1)], cw[(1, 1)] = torch.zeros_like(t[(0, 0)]), torch.zeros_like(aw), torch.zeros_like(aw), torch.zeros_like(aw)
        u1 = lambda a: a[..., None]                                                             # noqa: E731
        bil = sum(u1(cw[k]) * t[k] for k in cw)
        out += (u1(aw) * bil).sum(3)
        gw_l = (1 - ly) * ((1 - lx) * dot[(0, 0)] + lx * dot[(0, 1)]) + ly * ((1 - lx) * dot[(1, 0)] + lx * dot[(1, 1)])
        sx = (1 - ly) * (dot[(0, 1)] - dot[(0, 0)]) + ly * (dot[(1, 1)] - dot[(1, 0)])
        sy = (1 - lx) * (dot[(1, 0)] - dot[(0, 0)]) + lx * (dot[(1, 1)] - dot[(0, 1)])
        fx, fy = (1.0, 1.0) if wrong == "no_wh" else (float(W), float(H))
        gw[:, :, :, l, :] = gw_l * aw if wrong == "gw_times_w" else gw_l
        gl[:, :, :, l, :, 0], gl[:, :, :, l, :, 1] = aw * fx * sx, aw * fy * sy
        if want:
            sxc = u1(1 - ly) * (t[(0, 1)] - t[(0, 0)]) + u1(ly) * (t[(1, 1)] - t[(1, 0)])
            syc = u1(1 - lx) * (t[(1, 0)] - t[(0, 0)]) + u1(lx) * (t[(1, 1)] - t[(0, 1)])
            T.out += (u1(aw.abs()) * sum(u1(cw[k].abs()) * t[k].abs() for k in cw)).sum(3)
            T.c_out += (u1(aw.abs()) * (u1(ecx) * sxc.abs() + u1(ecy) * syc.abs())).sum(3)
            T.gw[:, :, :, l, :] = sum(cw[k].abs() * adot[k] for k in cw)
            T.c_gw[:, :, :, l, :] = ecx * sx.abs() + ecy * sy.abs()
            every = sum(dot[k].abs() for k in cw)
            T.gl[:, :, :, l, :, 0] = aw.abs() * W * ((1 - ly).abs() * (adot[(0, 1)] + adot[(0, 0)]) + ly.abs() * (adot[(1, 1)] + adot[(1, 0)]))
            T.gl[:, :, :, l, :, 1] = aw.abs() * H * ((1 - lx).abs() * (adot[(1, 0)] + adot[(0, 0)]) + lx.abs() * (adot[(1, 1)] + adot[(0, 1)]))
            T.c_gl[:, :, :, l, :, 0], T.c_gl[:, :, :, l, :, 1] = ecy * aw.abs() * W * every, ecx * aw.abs() * H * every
    return types.SimpleNamespace(out=out.reshape(bs, Q, heads * d), gv=gv.reshape(bs, S, heads, d), gl=gl, gw=gw, T=T, outside=outside)


def msda_reference(cs):
    """-> namespace: out, gv, gw with one bound each (the larger of the adjacent cells'), gl as a list of (ref, bound) per cell choice, and
    `outside` (samples whose contribution and gradients are exactly 0)"""
    bs, S, heads, d, Q, L, P = cs.dims
    near = [any(bool(msda_coords(cs, l)[4 + a].any()) for l in range(L)) for a in (0, 1)]
    alts = [(0, 0)] + [a for a in ((1, 0), (0, 1), (1, 1)) if all(near[i] or not a[i] for i in (0, 1))]
    E = [msda_eval(cs, F64, alt=a) for a in alts]
    n_red = (lambda t, r: (d + 10) * U * t) if cs.shuffle else (lambda t, r: A * t + 2.0 ** -20 * r.abs())
    mx = lambda ts: torch.stack(ts).max(0).values                                               # noqa: E731
    e0 = E[0]
    return types.SimpleNamespace(
        out=e0.out, b_out=mx([(L * P + 10) * U * e.T.out + e.T.c_out for e in E]).reshape(bs, Q, heads * d) + TINY,
        gv=e0.gv, b_gv=mx([A * e.T.gv + e.T.c_gv for e in E]).reshape(bs, S, heads, d) + 2.0 ** -20 * e0.gv.abs() + TINY,
        gw=e0.gw, b_gw=mx([n_red(e.T.gw, e.gw) + e.T.c_gw for e in E]) + TINY,
        gl=[e.gl for e in E], b_gl=[n_red(e.T.gl, e.gl) + e.T.c_gl + TINY for e in E],
        outside=e0.outside, alts=alts, shuffle=cs.shuffle)


def msda_check(ref, out=None, gv=None, gl=None, gw=None, what="msda"):
    """-> {name: worst error / bound} of the outputs given"""
    r = {}
    if out is not None:
        r["out"] = check_elements(out, ref.out, ref.b_out, f"{what} out")
    if gv is not None:
        r["grad_value"] = check_elements(gv, ref.gv, ref.b_gv, f"{what} grad_value")
    if gw is not None:
        r["grad_weight"] = check_elements(gw, ref.gw, ref.b_gw, f"{what} grad_weight")
    if gl is not None:
        r["grad_loc"] = check_any(gl, ref.gl, ref.b_gl, f"{what} grad_loc")
    return r


_LV1, _LV2 = [(1, 1)], [(1, 5), (5, 1)]
_LVP, _LV4 = [(8, 8), (4, 4), (2, 2), (1, 1)], [(13, 17), (7, 9), (4, 5), (2, 3)]
_ALL = MSDA_CLASSES
# bs Q heads d4 threads: 1 (one lane), 21, 56 and 63 (one partly filled wave, shuffle and atomic), 328 = 256 + 64 + 8 (a full block, a full
# wave and a ragged rest), 896, 38400 (150 blocks).  The grid cap of 65535 * 4 blocks needs more than 6.7e7 threads (a value tensor of
# gigabytes and seconds of float64 reference): out of reach of a seconds-sized test, not tested.
_MSDA = [
    dict(d=4, heads=1, bs=1, Q=1, P=1, levels=_LV1, classes=("inside",), seed=1),
    dict(d=4, heads=3, bs=1, Q=7, P=1, levels=_LV1, classes=_ALL, seed=2),
    dict(d=32, heads=1, bs=1, Q=7, P=3, levels=_LV2, classes=_ALL, seed=3),
    dict(d=12, heads=3, bs=1, Q=7, P=3, levels=_LV2, classes=_ALL, seed=4),                      # 63 threads, atomic path
    dict(d=4, heads=8, bs=1, Q=41, P=4, levels=_LV4, classes=_ALL, seed=5),                      # 328 threads
    dict(d=256, heads=1, bs=2, Q=7, P=3, levels=_LV2, classes=_ALL, seed=6),                     # the shuffle tree spans the wave
    dict(d=32, heads=8, bs=2, Q=300, P=4, levels=_LV4, classes=_ALL, seed=7),
    dict(d=32, heads=8, bs=1, Q=7, P=4, levels=_LVP, classes=_ALL, seed=8),                      # power-of-two levels: exact pixel centres
    dict(d=20, heads=3, bs=2, Q=7, P=4, levels=_LVP, classes=_ALL, seed=9),                      # atomic path
    dict(d=8, heads=3, bs=1, Q=300, P=3, levels=_LV2, classes=_ALL, seed=10),
    dict(d=8, heads=3, bs=2, Q=7, P=4, levels=_LVP, classes=("edge", "far"), only=1, seed=11),   # every sample outside, shuffle
    dict(d=12, heads=1, bs=1, Q=7, P=3, levels=_LV4[:2], classes=("edge", "far"), only=1, seed=12),   # every sample outside, atomic
]


# =================================================================================================== (h) ae_sam_pe_encode_f32
def pe_case(c):
    g = gen(c["seed"])
    H, W, F, N = c["H"], c["W"], c["F"], c["N"]
    xy = torch.rand(N, 2, generator=g) * torch.tensor([float(W), float(H)])
    xy[::3] = xy[::3].floor()                                                     # whole pixels beside fractional ones
    special = torch.tensor([[0.0, 0.0], [float(W), float(H)], [-10.5, H + 20.0], [W - 1.0, 0.25], [W + 0.5, -3.0], [0.0, float(H)]])
    if N == 1:
        xy[0] = special[3]
    else:
        xy[:6] = special
    labels = None
    if c["labels"]:
        labels = (torch.arange(N, dtype=torch.int32) % 5) - 1 if N > 1 else torch.tensor([1 if c["offset"] == 0 else -1], dtype=torch.int32)
    return xy.float(), randn(g, 2, F), labels, randn(g, 5, 2 * F)


def ref_pe(coords, gauss, H, W, offset, labels=None, table=None, variant=None):
    """sam_decoder.hip pe_encode_kernel's header -> (ref [N, 2F], bound)"""
    off, iw, ih = c32(offset), c32(1.0 / W), c32(1.0 / H)
    if variant == "swap_inv":
        iw, ih = ih, iw
    x, y = (coords[:, 0].to(F64) + off) * iw, (coords[:, 1].to(F64) + off) * ih
    g0, g1 = gauss[0].to(F64), gauss[1].to(F64)
    ph = 2.0 * math.pi * ((2 * x - 1)[:, None] * g0 + (2 * y - 1)[:, None] * g1)
    Pm = 2.0 * math.pi * ((2 * x.abs() + 1)[:, None] * g0.abs() + (2 * y.abs() + 1)[:, None] * g1.abs())
    enc, Pm = torch.cat([torch.sin(ph), torch.cos(ph)], 1), torch.cat([Pm, Pm], 1)
    if labels is None:
        return enc, U * (8 * Pm + 4 * enc.abs()) + TINY
    lab = labels.long()
    neg = (lab < 0)[:, None]
    if variant != "keep_neg":
        enc = torch.where(neg, torch.zeros_like(enc), enc)
    row = table.to(F64)[torch.where(lab < 0, torch.zeros_like(lab), 1 + lab) - (1 if variant == "row_off" else 0)]
    bnd = torch.where(neg, torch.full_like(enc, TINY), U * (8 * Pm + 4 * (enc.abs() + row.abs())) + TINY)
    return enc + row, bnd


# =================================================================================================== (i) ae_sam_mask_downscale_bf16
def downscale_case(c):
    g = gen(c["seed"])
    B, h, w = c["B"], c["h"], c["w"]
    m = (torch.rand(B, 1, 4 * h, 4 * w, generator=g) < 0.5).float() if c.get("binary") else randn(g, B, 1, 4 * h, 4 * w, scale=3.0)
    p = dict(w1=randn(g, 4, 1, 2, 2, scale=0.5), b1=randn(g, 4, scale=0.1), g1=1.0 + randn(g, 4, scale=0.3), e1=randn(g, 4, scale=0.2),
             w2=randn(g, 16, 4, 2, 2, scale=0.5), b2=randn(g, 16, scale=0.1), g2=1.0 + randn(g, 16, scale=0.3), e2=randn(g, 16, scale=0.2))
    # a zero and a small gain pin z near -2.9, where erf- and tanh-GELU differ by 4.4e-4: six times the bound's floor 2^-8 |gelu| + 1.13 a |z|
    p["g2"][5], p["e2"][5], p["g2"][12], p["e2"][12] = 0.0, -2.9, 0.05, -2.8
    return m, p


def _ln_stage(t, gam, bet, eps, dt, variant=None):
    """LayerNorm over the last dim of t with affine -> (z, Ez): Ez by family (i) with dt [..., 1] the error of t"""
    C = t.shape[-1]
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).sum(-1, keepdim=True) / (C - 1 if variant == "unbiased" else C)
    r = (var + eps).rsqrt()
    xh = (t - mu) * r
    e_r, e_mu = A, A * (1.0 + mu.abs() * r)
    Ez = gam.abs() * (xh.abs() * e_r + e_mu + r * (2.0 + xh.abs()) * dt) + A * (gam.abs() * r * (t.abs() + mu.abs()) + bet.abs())
    return xh * gam + bet, Ez


def ref_mask_downscale(m, p, eps=1e-6, variant=None):
    """conv k2s2 -> LN2d -> GELU -> conv k2s2 -> LN2d -> GELU, rows [B h w, 16] -> (ref, bound)"""
    B, _, H4, W4 = m.shape
    h, w = H4 // 4, W4 // 4
    q = {k: v.to(F64) for k, v in p.items()}
    eps = c32(eps)
    act = (lambda z: 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))) if variant == "tanh" else gelu64
    # [B, y, x, sy, sx, ky, kx]: pixel (4y + 2sy + ky, 4x + 2sx + kx)
    pt = m.to(F64).reshape(B, h, 2, 2, w, 2, 2).permute(0, 1, 4, 2, 5, 3, 6)
    w1 = q["w1"].reshape(4, 2, 2)
    t1 = torch.einsum("byxstkl,ckl->byxstc", pt, w1) + q["b1"]
    dt1 = 2.0 ** -22 * (torch.einsum("byxstkl,ckl->byxstc", pt.abs(), w1.abs()) + q["b1"].abs()).max(-1, keepdim=True).values
    z1, Ez1 = _ln_stage(t1, q["g1"], q["e1"], eps, dt1, variant)
    a1 = act(z1)
    t2 = torch.einsum("byxstc,ocst->byxo", a1, q["w2"]) + q["b2"]
    dt2 = (torch.einsum("byxstc,ocst->byxo", SLOPE_GELU * Ez1, q["w2"].abs())
           + A * (torch.einsum("byxstc,ocst->byxo", a1.abs(), q["w2"].abs()) + q["b2"].abs())).max(-1, keepdim=True).values
    z2, Ez2 = _ln_stage(t2, q["g2"], q["e2"], eps, dt2, variant)
    ref = act(z2).reshape(B * h * w, 16)
    return ref, BF_EPS * ref.abs() + SLOPE_GELU * Ez2.reshape(B * h * w, 16) + TINY


# =================================================================================================== (d) ae_sam_mask_product_f32
def product_case(c):
    g = gen(c["seed"])
    B, C, M, h, w = c["B"], c["C"], c["M"], c["h"], c["w"]
    return randn(g, B * h * w * 16, C, dtype=BF), randn(g, B, M, C)


def ref_mask_product(up, hyper, B, h, w, variant=None):
    """masks[b, m, Y, X] = sum_c hyper[b, m, c] up[b, pix(Y, X), c], pix = (((y w + x) 2 + dy1) 2 + dx1) 4 + 2 dy2 + dx2 with
    Y = 4y + 2 dy1 + dy2, X = 4x + 2 dx1 + dx2 -> (ref [B, M, 4h, 4w], bound)"""
    C = up.shape[1]
    Y, X = torch.meshgrid(torch.arange(4 * h), torch.arange(4 * w), indexing="ij")
    dy1, dy2 = (Y >> 1) & 1, Y & 1
    if variant == "swap_dy":
        dy1, dy2 = dy2, dy1
    pix = ((((Y >> 2) * w + (X >> 2)) * 2 + dy1) * 2 + ((X >> 1) & 1)) * 4 + dy2 * 2 + (X & 1)
    v = up.to(F64).reshape(B, 16 * h * w, C)[:, pix.reshape(-1)]                   # [B, 16 h w, C] in (Y, X) order
    hy = hyper.to(F64)
    if variant == "wrong_batch":
        hy = hy.roll(1, 0)
    ref = torch.einsum("bmc,bpc->bmp", hy, v).reshape(B, -1, 4 * h, 4 * w)
    terms = torch.einsum("bmc,bpc->bmp", hy.abs(), v.abs()).reshape(B, -1, 4 * h, 4 * w)
    return ref, bound_d(ref, terms)


# =================================================================================================== (h), (j) ae_sam_postprocess_masks
def _stage(n_in, n_out, align=False, unclamped=False):
    """F.interpolate(bilinear, align_corners=False) along one axis, n_in -> n_out: the interpolation matrix [n_out, n_in], the fp32
    allowance of the source coordinate [n_out], and the derivative matrices of the cell and of its two neighbours"""
    dst = torch.arange(n_out, dtype=F64)
    scale = n_in / n_out
    s = dst * ((n_in - 1) / max(n_out - 1, 1)) if align else (scale * (dst + 0.5) - 0.5).clamp(min=0.0)
    i0 = s.floor().long().clamp(max=n_in - 1)
    i1 = i0 + 1 if unclamped else i0 + (i0 < n_in - 1).long()
    l1 = s - i0
    Lm = torch.zeros(n_out, n_in + 1, dtype=F64)                                   # one spare column: the unclamped neighbour reads 0
    ar = torch.arange(n_out)
    Lm[ar, i0] += 1.0 - l1
    Lm[ar, i1] += l1
    ec = U * (2.0 * scale * (dst + 0.5) + s.abs())
    Ds = []
    for k in (-1, 0, 1):
        a, b = (i0 + k).clamp(0, n_in - 1), (i0 + k + 1).clamp(0, n_in - 1)
        D = torch.zeros(n_out, n_in, dtype=F64)
        D[ar, a] -= 1.0
        D[ar, b] += 1.0
        Ds.append(D)
    return Lm[:, :n_in], ec, Ds


def _resample(V, T, E, n_out_y, n_out_x, **kw):
    """one bilinear stage of V [N, Hin, Win] with its absolute terms T and inherited allowance E -> (V', T', E')"""
    Ly, ecy, Dy = _stage(V.shape[1], n_out_y, **kw)
    Lx, ecx, Dx = _stage(V.shape[2], n_out_x, **kw)
    f = lambda a, t, b: torch.einsum("yi,nij,xj->nyx", a, t, b)                    # noqa: E731
    R, Tn = f(Ly, V, Lx), f(Ly.abs(), T, Lx.abs())
    sy = torch.stack([f(D, V, Lx).abs() for D in Dy]).max(0).values
    sx = torch.stack([f(Ly, V, D).abs() for D in Dx]).max(0).values
    return R, Tn, f(Ly.abs(), E, Lx.abs()) + 2.0 ** -22 * Tn + ecy[None, :, None] * sy + ecx[None, None, :] * sx


def ref_postprocess(low, S, ih, iw, oh, ow, variant=None):
    """Sam.postprocess_masks: bilinear to S x S, crop to (ih, iw), bilinear to (oh, ow).  low [N, Hl, Wl] -> (logits [N, oh, ow], bound)"""
    V = low.to(F64)
    kw = dict(align=True) if variant == "align_corners" else dict(unclamped=True) if variant == "unclamped" else {}
    V1, T1, E1 = _resample(V, V.abs(), torch.zeros_like(V), S, S, **kw)
    if variant != "no_crop":
        V1, T1, E1 = V1[:, :ih, :iw], T1[:, :ih, :iw], E1[:, :ih, :iw]
    V2, _, E2 = _resample(V1, T1, E1, oh, ow, **kw)
    return V2, E2 + TINY


def postprocess_mask(ref, bnd, thr, merge):
    """-> (mask uint8, decided bool): [N, oh, ow], or [oh, ow] for the merged union"""
    t = c32(thr)
    above, below = ref - t > bnd, t - ref >= bnd
    if not merge:
        return (ref > t).to(torch.uint8), above | below
    return (ref > t).any(0).to(torch.uint8), above.any(0) | below.all(0)


def check_mask(got, mask, decided, what):
    bad = (got != mask) & decided
    if got.shape != mask.shape or bool(bad.any()) or bool((got > 1).any()):
        raise BoundFailure(f"{what}: {int(bad.sum())} of {int(decided.sum())} decided pixels differ (shape {tuple(got.shape)})")
    return 0.0


def postprocess_case(c):
    return randn(gen(c["seed"]), c["N"], *c["low"], scale=3.0)


# =================================================================================================== (j) ae_sam_preprocess_f32
def preprocess_case(c):
    g = gen(c["seed"])
    B, C, h, w = 2, c["C"], c["h"], c["w"]
    x = torch.randint(0, 256, (B, C, h, w), generator=g).to(torch.uint8) if c["u8"] else randn(g, B, C, h, w, scale=80.0) + 120.0
    return x, torch.tensor([123.675, 116.28, 103.53][:C]), torch.tensor([58.395, 57.12, 57.375][:C])


def ref_preprocess(x, S, mean, std):
    """(x - mean[c]) / std[c], zero-padded right / bottom to S x S -> (ref, bound, padding mask)"""
    B, C, h, w = x.shape
    xx, mu, sd = x.to(F64), mean.to(F64).reshape(1, C, 1, 1), std.to(F64).reshape(1, C, 1, 1)
    ref, bnd = torch.zeros(B, C, S, S, dtype=F64), torch.full((B, C, S, S), TINY, dtype=F64)
    ref[:, :, :h, :w] = (xx - mu) / sd
    bnd[:, :, :h, :w] = 2.0 ** -22 * (xx.abs() + mu.abs()) / sd.abs() + TINY
    pad = torch.ones(B, C, S, S, dtype=torch.bool)
    pad[:, :, :h, :w] = False
    return ref, bnd, pad


# =================================================================================================== (j) ae_nms_sorted_f32
def nms_case(c):
    """boxes [N, 4] fp32 XYXY in the order the kernel visits them"""
    kind = c["kind"]
    if kind == "random":
        g = gen(c["seed"])
        N = c["N"]
        ctr = torch.rand(N, 2, generator=g) * 1000.0
        wh = 10.0 + torch.rand(N, 2, generator=g) * 90.0
        return torch.cat([ctr - wh / 2, ctr + wh / 2], 1).float()
    built = {
        "tie": [[0, 0, 4, 4], [0, 0, 4, 2], [0, 0, 2, 4], [8, 8, 16, 16], [8, 8, 16, 12]],            # IoU exactly 0.5 = the threshold: kept
        "duplicates": [[1, 1, 5, 6], [1, 1, 5, 6], [10, 10, 12, 12], [1, 1, 5, 6], [10, 10, 12, 12]],
        "zero_area": [[0, 0, 4, 4], [2, 2, 2, 2], [2, 2, 2, 2], [1, 1, 1, 3], [0, 0, 4, 4], [7, 7, 7, 7]],
        "chain": [[0, 0, 10, 10], [0, 0, 8, 8], [0, 0, 6, 6]],                                         # B falls to A; C overlaps only B: kept
        "equal_scores": [[0, 0, 4, 4], [0, 0, 4, 3.5], [5, 5, 9, 9], [0, 0, 3.9, 4], [5, 5, 9, 8.5]],
    }
    return torch.tensor(built[kind], dtype=F32)


def nms_iou(boxes, rows):
    """float64 IoU of boxes[rows] against all boxes, the kernel's expression (0 / 0 = NaN compares false)"""
    b = boxes.to(F64)
    a = b[rows]
    iw = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area[rows][:, None] + area[None, :] - inter)


def ref_nms(boxes, thr, variant=None):
    """box i survives unless an earlier SURVIVOR overlaps it with IoU > thr -> keep [N] uint8"""
    N, t = boxes.shape[0], c32(thr)
    removed = torch.zeros(N, dtype=torch.bool)
    later = torch.arange(N)
    for i in range(N):
        if removed[i] and variant != "by_removed":
            continue
        iou = nms_iou(boxes, torch.tensor([i]))[0]
        removed |= ((iou >= t) if variant == "ge" else (iou > t)) & (later > i)
    return (~removed).to(torch.uint8)


# =================================================================================================== the cases
_POST_GEO = [dict(low=(8, 8), S=32, inp=(32, 21), orig=(50, 37)), dict(low=(8, 8), S=32, inp=(20, 32), orig=(9, 40)),
             dict(low=(1, 6), S=24, inp=(24, 24), orig=(1, 1)), dict(low=(4, 4), S=16, inp=(16, 16), orig=(16, 16))]
_POST_MODE = [dict(mode="logits", N=3, thr=0.0), dict(mode="mask", N=3, thr=0.0), dict(mode="both", N=3, thr=0.7),
              dict(mode="merge", N=1, thr=0.0), dict(mode="merge", N=3, thr=0.7)]

CASES = {
    # ---- msda.hip
    "ae_linear_f32": (_prod(M=[1, 31, 64, 65], N=[1, 4, 33, 64, 65], K=[16, 48, 256], bias=[0, 1])
                      + [dict(M=65, N=33, K=48, bias=1, lda=52, ldw=56, ldc=40)]),
    "ae_ms_deform_attn_fwd_f32": _MSDA,
    "ae_ms_deform_attn_bwd_f32": _MSDA,
    # ---- sam_decoder.hip
    "ae_sam_pe_encode_f32": [dict(H=h, W=w, F=f, N=n, offset=o, labels=lb, seed=200 + i) for i, (h, w) in enumerate(((64, 64), (48, 80), (1024, 683)))
                             for f in (1, 3, 128) for n in (1, 257) for o in (0.0, 0.5) for lb in (0, 1)],
    "ae_sam_mask_downscale_bf16": [dict(B=b, h=h, w=w, seed=300 + i) for i, (b, h, w) in enumerate(((1, 1, 1), (1, 3, 5), (2, 16, 24), (3, 17, 15)))]
                                  + [dict(B=2, h=16, w=24, binary=1, seed=304)],
    "ae_sam_mask_product_f32": ([dict(C=cc, M=m, B=b, h=h, w=w, seed=400 + cc + m) for cc in (8, 16, 32, 64) for m in (1, 2, 5, 8) for b in (1, 3)
                                 for (h, w) in ((1, 1), (5, 7))]
                                + [dict(C=8, M=1, B=1, h=PRODUCT_WRAP[0], w=PRODUCT_WRAP[1], seed=499, wrap=True)]),
    "ae_nms_sorted_f32": ([dict(kind="random", N=n, thr=t, seed=500 + n % 97) for n in (1, 2, 256, 257, 3855, 3856, 8192) for t in (0.3, 0.5)]
                          + [dict(kind=k, thr=0.5) for k in ("tie", "duplicates", "zero_area", "chain", "equal_scores")]),
    "ae_sam_postprocess_masks": [dict(g, **m, seed=600 + 10 * i + j) for i, g in enumerate(_POST_GEO) for j, m in enumerate(_POST_MODE)],
    "ae_sam_preprocess_f32": [dict(u8=u, C=cc, h=h, w=w, S=s, seed=700 + cc) for u in (0, 1) for cc in (1, 3) for (h, w, s) in ((5, 7, 8), (8, 8, 8), (1, 8, 8))],
}
SOURCES = ("msda.hip", "sam_decoder.hip")
NMS_MAX = 8192                     # the documented limit of ae_nms_sorted_f32 (139 264 bytes of LDS)
