"""Route cases of gemm_conv.hip / attention_fast.hip on the GPU: which instantiation ran, and is every checked output element right.

For each case of tests/route_cases.py (one process, run with no AE_* routing variable set; tests/test_kernel_routes.py starts it that way):
  1. seeded bf16 operands; the op runs through `ops` once under torch.profiler (device activity) -> the kernel names of that case;
  2. the case must reach every instantiation whose `default` ledger row lists it, and the library's own report of its plan (`ops.conv_plan` /
     `ops.up2_plan` / `ops.gemm_plan`: the launch selection run without launching) must name what ran: all twelve template arguments of the
     gemm_kernel, a split plan <=> the split-K reduce ran (the factor equal to what `ae_conv3x3_workspace_floats` sizes), the stand-alone
     column-statistics kernel <=> the report says so;
  3. every output (and column / row statistics buffer) is a view of a larger allocation whose guard areas — rows before and after, columns past
     N where the op takes a row stride, slabs past ceil(M / 32) — hold a sentinel bit pattern that must be unchanged after the launch;
  4. a second run (fresh guarded buffers) must be bit-identical;
  5. the output is compared with a float64 CPU reference on the same bf16 operands, element by element, on a row subset that holds every
     structurally special row: the first and last 192-row tile, the ragged tail, the rows within one image row of sample boundaries and of tile
     boundaries that fall inside an image row, and 512 seeded random rows (attention: the last 128-query block, the first 32 queries and 256
     random ones, on four (batch, head) pairs).  The boundary windows are all checked while each kind stays within a row budget (1024-8192
     rows, by the case's K x N); cases with more boundaries than that (the short-map and many-tile cases) check the first, the last and a
     seeded random subset of them — a narrowing of "every boundary", bounded by the CPU time of the float64 reference.

Bound.  GEMM / conv outputs (bf16): |got - ref| <= 2^-8 |ref| + a * (|A| |W|)[row, col] with a = 2^-16: the first term is one bf16 rounding
of the output (round-to-nearest: half an ulp = 2^-8 relative at most), the second the fp32 accumulation; |A| |W| is the float64 product of the
absolute operands of the same row and column (for split-K the fp32 partials and their fp32 reduce are inside the same term).  An fp32
accumulator of K bf16 products has a worst-case error of ~K 2^-24 |A||W| and a random-walk error of ~sqrt(K) 2^-24 |A||W|: a = 2^-16 is 256
times the unit roundoff, above the random walk for every K here (sqrt(23040) = 152) and far below one bf16 ulp of a typical output, so one
wrong tap, one wrong K range or a wrong row fails it.  fp32 outputs: 2^-20 |ref| + a |A||W|.  GELU / GEGLU: the a-term is carried through the
activation's slope (|gelu'| <= 1.13).  LayerNorm fold: a * rstd * (|x| |W| + |mean| |s|).  Column / row statistics: the float64 sums of the
STORED bf16 output per slab, |got - ref| <= a * sum|y| (resp. sum y^2) + 1e-30.  Attention: 2^-8 |ref| + 2^-8 * sum_j p_j |v_j| — the
probabilities enter the PV product as bf16 (half an ulp each), the logits and the normalisation are fp32.

Bound, log-sum-exp.  Every attention case also asks for `lse` (and `lse2` when it has a second segment) in the launches above: fp32
[B, H, Nq], L2 = log2 sum_j exp(S_j) with S the logits in natural units (scale q.k + rel-pos bias; for lse2 the second segment's own
logits with the same scale — scale2 is the gate on the output and does not enter).  The buffers sit between guards like the output, must
repeat bit for bit and must hold no sentinel afterwards (every (b, h, q) was written).  On the checked (batch, head) pairs and query rows
    |got - L2| <= log2(e) * (2^-8 + (a + 2^-9) * scale * max_j sum_d |q_d| |k_jd| + [rel-pos only] 2^-9 (max|rel_h| + max|rel_w|))
                  + 2^-22 |L2| + 1e-6.
The log-sum-exp is 1-Lipschitz in the sup-norm of the logits, so a per-logit error enters once, whatever the number of keys: the a-term
is the fp32 accumulation of a logit (the constant of the output bound), the bias term the bf16 bias operands of the BIAS 3 route (as in
the output bound).  2^-9 scale sum_d |q_d| |k_jd|: every kernel of attention_fast.hip multiplies Q by scale log2(e) ONCE and rounds the
product to bf16 for the logit MFMA (its header, "Q is pre-multiplied"; load_q: pack_bf16x2(q * c)), half an ulp = 2^-9 relative per
factor, so a logit is off by up to 2^-9 of its absolute products.  (Measured without this term on the MI355X: the short-K/V two-segment
routes reached 1.7 times the bound on a second segment of 8 or 16 keys, where nothing averages the rounding out, and every other route
0.12 - 0.98.)  2^-8: the fast kernels' denominator is a row of the PV MFMA, i.e. a sum of bf16-rounded probabilities — each within
2^-8 relative (round-to-nearest: half an ulp; a truncating conversion is within one ulp, 2^-8 relative on average over a binade), all
non-negative, so their sum is too, and |log(1 + x)| <= |x| / (1 - |x|); the general kernel sums fp32 probabilities and sits far below it.  2^-22 |L2| + 1e-6: the fp32 store of offset + log2(denominator) and the hardware exp2 / log2 (about 1 ulp each).  The worst
ratio of a case is printed as `lse_ratio`.

    python tools/route_check.py [case-id-substring ...]      # prints one line per case, then `ROUTE_SUMMARY {json}`
"""
import json
import os
import re
import subprocess
import sys
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import route_cases as RC  # noqa: E402

BF = torch.bfloat16
F64 = torch.float64
A_ACC = 2.0 ** -16
BF_SENT, F32_SENT = 0x7FA5, 0x7FA5A5A5          # NaN bit patterns no kernel writes
GUARD_ROWS = 64
FAMILIES = re.compile(r"\b(gemm_kernel|attn_fast_kernel|attn_pipe_kernel)<([^<>]*)>")


class CaseFailure(Exception):
    pass


# --------------------------------------------------------------------------------------------------- guarded outputs
class Guarded:
    """`rows` x `cols` view (row stride `ld`) inside a flat allocation with GUARD elements before and after, sentinel-filled."""

    def __init__(self, rows, cols, dtype, ld=None, col0=0, guard=None, trailing=()):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.ld = ld or cols
        inner = int(torch.tensor(trailing).prod()) if trailing else 1
        g = guard if guard is not None else GUARD_ROWS * self.ld * inner
        self.off = g + col0 * inner
        n = g + rows * self.ld * inner + g
        self.buf = torch.empty(n, dtype=dtype, device="cuda")
        self.int_view = self.buf.view(torch.int16 if dtype == BF else torch.int32)
        self.sent = BF_SENT if dtype == BF else F32_SENT
        self.int_view.fill_(self.sent)
        self.trailing = tuple(trailing)
        self.view = self.buf.as_strided((rows, cols) + self.trailing, (self.ld * inner, inner) + tuple(self._tstride()), self.off)

    def _tstride(self):
        s, out = 1, []
        for d in reversed(self.trailing):
            out.insert(0, s)
            s *= d
        return out

    def guards_intact(self):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        idx = torch.arange(self.buf.numel(), device="cuda").as_strided(self.view.shape, self.view.stride(), self.off)
        mask[idx.reshape(-1)] = False
        return bool((self.int_view[mask] == self.sent).all())

    def bits(self):
        return self.view.contiguous().view(torch.int16 if self.dtype == BF else torch.int32).cpu()


# --------------------------------------------------------------------------------------------------- row subsets
def pick_rows(M, rows_per_sample, width, gen, tile=192, budget=8192):
    """Row subset for the float64 reference (see the module docstring).  The windows of one image row around every sample boundary and every
    in-row tile boundary are all taken while each kind stays within `budget` rows; past that, the first, the last and seeded random
    boundaries up to the budget."""
    r = set(range(min(tile, M))) | set(range(max(0, M - tile), M)) | set(range(M // tile * tile, M))
    bounds = [b * rows_per_sample for b in range(1, M // rows_per_sample)] if rows_per_sample else []
    tb = [t * t_ for t_ in (192, 128) for t in range(1, (M - 1) // t_ + 1) if width and (t * t_) % width]
    w = width or 1
    for lst in (bounds, tb):
        k = max(2, budget // (2 * w))
        sel = lst if len(lst) <= k else [lst[0], lst[-1]] + [lst[int(i)] for i in torch.randperm(len(lst), generator=gen)[:k - 2]]
        for c in sel:
            r |= set(range(max(0, c - w), min(M, c + w)))
    r |= set(int(i) for i in torch.randint(0, M, (512,), generator=gen))
    return torch.tensor(sorted(r), dtype=torch.long)


def row_budget(K, N):
    """rows per boundary kind: ~3e10 multiply-adds of float64 reference (and as many for |A| |W|) per kind, between 1024 and 8192 rows"""
    return int(min(8192, max(1024, 3e10 / (K * N))))


def bound_check(got, ref, bnd, what):
    err = (got.to(F64) - ref).abs()
    if not torch.isfinite(got).all():
        raise CaseFailure(f"{what}: non-finite values in the checked rows")
    ratio = float((err / bnd).max())
    if ratio > 1.0:
        i = int((err / bnd).flatten().argmax())
        r, c = divmod(i, ref.shape[-1])
        raise CaseFailure(f"{what}: element ({r}, {c}) got {float(got.flatten()[i]):.6g} ref {float(ref.flatten()[i]):.6g} "
                          f"err {float(err.flatten()[i]):.3g} > bound {float(bnd.flatten()[i]):.3g} (ratio {ratio:.2f})")
    return ratio


def stats_check(got, y, slab_rows, what, per_row=False, sample_rows=0):
    """got: fp32 statistics buffer; y: the stored bf16 output (CPU).  Column statistics [ceil(M/32), N, 2] per 32-row slab, row statistics
    [M, N/64, 2] per 64-column slice.  sample_rows: compare per-sample totals of the slabs (conv3x3_up2 keeps its slabs per sample and
    output parity, not per 32 consecutive rows; its consumer only sums a sample's slabs)."""
    y = y.to(F64)
    if sample_rows:
        M, N = y.shape
        yy = y.reshape(M // sample_rows, sample_rows, N)
        s, q, sa = yy.sum(1), (yy * yy).sum(1), yy.abs().sum(1)
        got = got.reshape(M // sample_rows, sample_rows // slab_rows, N, 2).sum(1)
    elif per_row:
        M, N = y.shape
        yy = y.reshape(M, N // 64, 64)
        s, q, sa = yy.sum(-1), (yy * yy).sum(-1), yy.abs().sum(-1)
    else:
        M, N = y.shape
        S = (M + slab_rows - 1) // slab_rows
        pad = torch.zeros(S * slab_rows - M, N, dtype=F64)
        yy = torch.cat([y, pad]).reshape(S, slab_rows, N)
        s, q, sa = yy.sum(1), (yy * yy).sum(1), yy.abs().sum(1)
    r1 = bound_check(got[..., 0], s, A_ACC * sa + 1e-30, what + " sums")
    r2 = bound_check(got[..., 1], q, A_ACC * q + 1e-30, what + " sums of squares")
    return max(r1, r2)


# --------------------------------------------------------------------------------------------------- kernel names
def route_keys(names, families=None):
    """kernel names of a profiler capture -> (demangled names, ledger keys); families: the regular expression of another file's kernel templates"""
    families = families or FAMILIES
    mangled = [n for n in names if n.startswith("_Z")]
    if mangled:
        dm = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
        table = dict(zip(mangled, dm))
        names = [table.get(n, n) for n in names]
    keys = []
    for n in names:
        m = families.search(n)
        if m:
            keys.append(f"{m.group(1)}<{', '.join(x.strip() for x in m.group(2).split(','))}>")
        elif "splitk_reduce_kernel" in n:
            keys.append("splitk_reduce_kernel")
        elif "colstats_kernel" in n:
            keys.append("colstats_kernel")
    return names, keys


def profiled(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = []
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name not in names:
            names.append(e.name)
    return out, names


# --------------------------------------------------------------------------------------------------- operands
def rnd(gen, *shape, scale=1.0, mean=0.0):
    return (torch.randn(*shape, generator=gen) * scale + mean).to(BF)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2 ** 0.5))


def run_conv(c, ops, gen):
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    s, ups = c.get("stride", 1), c.get("ups", 0)
    Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (Hv - 1) // s + 1, (Wv - 1) // s + 1
    M = B * Ho * Wo
    x = rnd(gen, B * H * W, Cin)
    w = rnd(gen, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5)
    bias = torch.randn(Cout, generator=gen) * 0.1
    addvec = torch.randn(B, Cout, generator=gen) * 0.1 if c.get("addvec") else None
    res = rnd(gen, M, Cout) if c.get("res") else None
    k = c.get("k")
    if k is None:
        k = ops.conv_k_order(M, Cin, Cout, s, bool(ups))
    wp = ops.pack_conv3x3(w, k_order=k)
    f32 = c.get("f32", False)
    dev = [t.cuda() if t is not None else None for t in (x, wp, bias, addvec, res)]
    cs = c.get("cs", False)

    def launch():
        o = Guarded(M, Cout, torch.float32 if f32 else BF)
        st = _stats_with_tail((M + 31) // 32, Cout) if cs else None
        ops.conv3x3(dev[0], dev[1], dev[2], B, H, W, addvec=dev[3], residual=dev[4], stride=s, upsample2x=ups, out_f32=f32,
                    out=o.view, colstats=st.view if st is not None else None, k_order=k)
        return o, st

    # reference rows
    rows = pick_rows(M, Ho * Wo, Wo, gen, budget=row_budget(9 * Cin, Cout))
    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    yo, xo = rem // Wo, rem % Wo
    xf = x.to(F64).reshape(B, H, W, Cin)
    P = torch.zeros(len(rows), 9, Cin, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            yv, xv = yo * s + ky - 1, xo * s + kx - 1
            ok = (yv >= 0) & (yv < Hv) & (xv >= 0) & (xv < Wv)
            if ups == 2:
                ok &= (yv % 2 == 0) & (xv % 2 == 0)
            ys, xs = (yv.clamp(0, Hv - 1) // 2, xv.clamp(0, Wv - 1) // 2) if ups else (yv.clamp(0, H - 1), xv.clamp(0, W - 1))
            P[:, 3 * ky + kx] = xf[b, ys, xs] * ok[:, None]
    Wt = w.to(F64).permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    P = P.reshape(len(rows), 9 * Cin)
    ref = P @ Wt.t() + bias.to(F64)
    if addvec is not None:
        ref += addvec.to(F64)[b]
    if res is not None:
        ref += res.to(F64)[rows]
    absprod = P.abs() @ Wt.abs().t()
    bnd = (2.0 ** -20 if f32 else 2.0 ** -8) * ref.abs() + A_ACC * absprod + 1e-30
    nws = ops.lib.ae_conv3x3_workspace_floats(B, H, W, Cin, Cout, s, int(ups))
    return dict(launch=launch, rows=rows, ref=ref, bnd=bnd, cs=cs, M=M, N=Cout, conv=True, f32=f32,
                plan=lambda: ops.conv_plan(B, H, W, Cin, Cout, s, ups, f32, cs, k), ws_split=nws // (M * Cout) if nws else 1)


def _stats_with_tail(S, N, tail=4):
    """column-statistics buffer [S, N, 2] followed by `tail` guard slabs (its own allocation: the op wants a contiguous view)"""
    t = Guarded(S + tail, N, torch.float32, guard=0, trailing=(2,))
    t.view = t.buf.as_strided((S, N, 2), (2 * N, 2, 1), 0)
    return t


def run_up2(c, ops, gen):
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    M = B * 4 * H * W
    x = rnd(gen, B * H * W, Cin)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (9 * Cin) ** -0.5
    w4 = ops.pack_conv3x3_up2(w)
    bias = torch.randn(Cout, generator=gen) * 0.1
    dev = [x.cuda(), w4.cuda(), bias.cuda()]
    cs = c["cs"]

    def launch():
        o = Guarded(M, Cout, BF)
        st = _stats_with_tail((M + 31) // 32, Cout) if cs else None
        ops.conv3x3_up2(dev[0], dev[1], dev[2], B, H, W, out=o.view, colstats=st.view if st is not None else None)
        return o, st

    Ho, Wo = 2 * H, 2 * W
    rows = pick_rows(M, Ho * Wo, Wo, gen, budget=row_budget(4 * Cin, Cout))
    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    Y, X = rem // Wo, rem % Wo
    y, py, xx, px = Y // 2, Y % 2, X // 2, X % 2
    xf = x.to(F64).reshape(B, H, W, Cin)
    w4f = w4.to(F64).reshape(4, Cout, 4, Cin)
    ref = torch.zeros(len(rows), Cout, dtype=F64) + bias.to(F64)
    absprod = torch.zeros(len(rows), Cout, dtype=F64)
    for par in range(4):
        sel = (2 * py + px) == par
        if not sel.any():
            continue
        P = torch.zeros(int(sel.sum()), 4, Cin, dtype=F64)
        for i in range(2):
            for j in range(2):
                ys, xs = y[sel] + par // 2 - 1 + i, xx[sel] + par % 2 - 1 + j
                ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
                P[:, 2 * i + j] = xf[b[sel], ys.clamp(0, H - 1), xs.clamp(0, W - 1)] * ok[:, None]
        Wt = w4f[par].reshape(Cout, 4 * Cin)
        P = P.reshape(-1, 4 * Cin)
        ref[sel] += P @ Wt.t()
        absprod[sel] = P.abs() @ Wt.abs().t()
    bnd = 2.0 ** -8 * ref.abs() + A_ACC * absprod + 1e-30
    return dict(launch=launch, rows=rows, ref=ref, bnd=bnd, cs=cs, M=M, N=Cout, conv=True, f32=False, sample_rows=Ho * Wo,
                plan=lambda: ops.up2_plan(B, H, W, Cin, Cout, cs))


def run_gemm(c, ops, gen, ln=False):
    M, N, K = c["M"], c["N"], c["K"]
    epi = {"none": ops.EPI_NONE, "gelu": ops.EPI_GELU, "geglu": ops.EPI_GEGLU}[c.get("epi", "none")]
    n_out = N // 2 if epi == ops.EPI_GEGLU else N
    a = rnd(gen, M, K, mean=0.3 if ln else 0.0)
    w = rnd(gen, N, K, scale=K ** -0.5)
    bias = torch.randn(N, generator=gen) * 0.1 if (c.get("bias") or ln) else None
    res = rnd(gen, M, n_out) if c.get("res") else None
    f32, cs, rs = c.get("f32", False), c.get("cs", False), c.get("rs", False)
    a2k = c.get("a2")
    cpad = c.get("cpad", 0)
    eps = 1e-5
    af = a.to(F64)
    if ln:
        mu, var = af.mean(1), af.var(1, unbiased=False)
        rstd = (var + eps).rsqrt()
        sl = af.reshape(M, K // 64, 64)
        ln_stats = torch.stack([sl.sum(-1), (sl * sl).sum(-1)], -1).float().contiguous()
        s_col = w.to(F64).sum(1).float()
        dev_ln = (ln_stats.cuda(), s_col.cuda())
    dev_a = a.cuda()
    dev = [dev_a[:, :a2k] if a2k else dev_a, dev_a[:, a2k:] if a2k else None, w.cuda(),
           bias.cuda() if bias is not None else None, res.cuda() if res is not None else None]

    def launch():
        col0 = 8 if cpad else 0
        o = Guarded(M, n_out, torch.float32 if f32 else BF, ld=n_out + cpad + col0, col0=col0)
        st = _stats_with_tail((M + 31) // 32, n_out) if cs else None
        rsb = None
        if rs:
            rsb = Guarded(M, N // 64, torch.float32, trailing=(2,))
        if ln:
            ops.gemm_ln(dev[0], dev_ln[0], dev[2], dev_ln[1], dev[3], eps, residual=dev[4], epilogue=epi, out=o.view)
        elif rs:
            ops.gemm(dev[0], dev[2], bias=dev[3], residual=dev[4], out=o.view, rowstats=rsb.view)
        else:
            ops.gemm(dev[0], dev[2], bias=dev[3], residual=dev[4], epilogue=epi, out_f32=f32, a2=dev[1], out=o.view,
                     colstats=st.view if st is not None else None)
        return o, st if not rs else rsb

    rows = pick_rows(M, 0, 0, gen)
    Ar, Wf = af[rows], w.to(F64)
    y = Ar @ Wf.t()
    absprod = Ar.abs() @ Wf.abs().t()
    if ln:
        y = rstd[rows, None] * (y - mu[rows, None] * Wf.sum(1)[None, :])
        absprod = rstd[rows, None] * (absprod + mu[rows, None].abs() * Wf.abs().sum(1)[None, :])
    if bias is not None:
        y = y + bias.to(F64)
    if epi == ops.EPI_GELU:
        ref, acc = gelu64(y), 1.13 * A_ACC * absprod
    elif epi == ops.EPI_GEGLU:
        R = len(rows)
        ya, yg = y.reshape(R, N // 32, 2, 16).unbind(2)
        pa, pg = absprod.reshape(R, N // 32, 2, 16).unbind(2)
        ref = (ya * gelu64(yg)).reshape(R, n_out)
        acc = A_ACC * (gelu64(yg).abs() * pa + 1.13 * ya.abs() * pg).reshape(R, n_out)
    else:
        ref, acc = y, A_ACC * absprod
    if res is not None:
        ref = ref + res.to(F64)[rows]
    bnd = (2.0 ** -20 if f32 else 2.0 ** -8) * ref.abs() + acc + 1e-30
    return dict(launch=launch, rows=rows, ref=ref, bnd=bnd, cs=cs, rs=rs, M=M, N=n_out, conv=False, f32=f32,
                plan=lambda: ops.gemm_plan(M, N, K, epi, a2k or 0, f32, cs, 2 if ln else 1 if rs else 0))


LOG2E = 1.4426950408889634


def attn_segment_ref(qq, K, V, scale, bias=None, live=None):
    """float64 reference of one attention segment of one (batch, head): qq [n, D] query rows, K / V [Nk, D]; bias = (rel_h [n, kH], rel_w [n, kW])
    of the same rows; live = bool [Nk], False = a key the mask removes (masked_fill(-finfo.max) before the softmax, so a row with no live key is
    the plain mean of the value rows).  Returns r = softmax(S) V, sv = softmax(S) |V|, bmax = max|rel_h| + max|rel_w| per row (None without a
    bias), and L2 / L2_bnd: the log2-domain log-sum-exp over the live keys and its bound (module docstring; None when no key is live)."""
    S = (qq @ K.t()) * scale
    qk_abs = qq.abs() @ K.abs().t()
    bmax = None
    if bias is not None:
        rh, rw = bias
        S = S + rh.repeat_interleave(rw.shape[1], 1) + rw.repeat(1, rh.shape[1])
        bmax = (rh.abs().max(1).values + rw.abs().max(1).values)[:, None]
    Sl = S
    if live is not None:
        Sl, qk_abs = S[:, live], qk_abs[:, live]
        S = S.masked_fill(~live[None, :], -torch.finfo(S.dtype).max)
    L2 = lb = None
    if Sl.shape[1]:
        L2 = torch.logsumexp(Sl, -1) * LOG2E
        per_logit = 2.0 ** -8 + (A_ACC + 2.0 ** -9) * scale * qk_abs.max(1).values
        if bmax is not None:
            per_logit = per_logit + 2.0 ** -9 * bmax[:, 0]
        lb = LOG2E * per_logit + 2.0 ** -22 * L2.abs() + 1e-6
    p = torch.softmax(S, -1)
    return dict(r=p @ V, sv=p @ V.abs(), bmax=bmax, L2=L2, L2_bnd=lb)


def attn_out_bound(r, sv, bmax=None, stored=None, gate=1.0):
    """bound of the bf16 attention output: one rounding of the stored value (r, or `stored` = prev + gate r under accumulate / out_scale) and one
    of each probability; with a rel-pos bias each logit may be off by 2^-9 (|rel_h| + |rel_w|) (BIAS 3 of attention_fast.hip: bf16 bias operands)"""
    g = abs(gate)
    bnd = 2.0 ** -8 * (r if stored is None else stored).abs() + g * 2.0 ** -8 * sv
    if bmax is not None:
        bnd = bnd + g * 2.0 ** -9 * bmax * (sv + r.abs())
    return bnd + 1e-30


def run_attn(c, ops, gen):
    B, H, Nq, Nk, D = c["B"], c["H"], c["Nq"], c["Nk"], c["D"]
    C = H * D
    scale = D ** -0.5
    nk2 = c.get("nk2")
    rel = c.get("rel")
    if c["lay"] == "qkv":
        if Nq == Nk and not nk2:     # self-attention on fused qkv rows [B*N, 3C]
            qkv = rnd(gen, B * Nq, 3 * C)
            q, k, v = qkv, qkv[:, C:], qkv[:, 2 * C:]
            st = (Nq * 3 * C, D, 3 * C)
            qs = ks = vs = st
            qc = qkv.cuda()
            dq, dk, dv = qc, qc[:, C:], qc[:, 2 * C:]
        else:                        # q rows [B*Nq, C] + packed kv rows [B*Nk, 2C]
            q = rnd(gen, B * Nq, C)
            kv = rnd(gen, B * Nk, 2 * C)
            k, v = kv, kv[:, C:]
            qs, ks = (Nq * C, D, C), (Nk * 2 * C, D, 2 * C)
            vs = ks
            kvc = kv.cuda()
            dq, dk, dv = q.cuda(), kvc, kvc[:, C:]
    else:
        q, k, v = rnd(gen, B * H, Nq, D), rnd(gen, B * H, Nk, D), rnd(gen, B * H, Nk, D)
        qs, ks, vs = (H * Nq * D, Nq * D, D), (H * Nk * D, Nk * D, D), (H * Nk * D, Nk * D, D)
        dq, dk, dv = q.cuda(), k.cuda(), v.cuda()

    def view4(t, n, st):   # (B, H, n, D) float64 view of a strided operand
        return t.as_strided((B, H, n, D), st + (1,), t.storage_offset()).to(F64)

    seg = None
    if nk2:
        k2 = rnd(gen, B * nk2, 2 * C)
        st2 = (nk2 * 2 * C, D, 2 * C)
        s2 = torch.linspace(0.5, 1.5, B)
        k2c = k2.cuda()
        seg = (k2c, k2c[:, C:], nk2, st2, st2, s2.cuda())
    relh = relw = None
    if rel:
        kH, kW = rel
        relh = torch.randn(B * H, Nq, kH, generator=gen)
        relw = torch.randn(B * H, Nq, kW, generator=gen)
    dev_rel = (relh.cuda(), relw.cuda()) if rel else (None, None)
    total = B * Nq * C
    g = 4096

    def launch():
        o = Guarded(1, total, BF, guard=g)
        ov = o.view.reshape(B, Nq, C)
        ls = [Guarded(1, B * H * Nq, torch.float32, guard=g) for _ in range(2 if nk2 else 1)]
        ops.attention(dq, dk, dv, B, H, Nq, Nk, D, scale, qs, ks, vs, out=ov, rel_h=dev_rel[0], rel_w=dev_rel[1],
                      kH=rel[0] if rel else 0, kW=rel[1] if rel else 0, seg2=seg, lse=ls[0].view.reshape(B, H, Nq),
                      lse2=ls[1].view.reshape(B, H, Nq) if nk2 else None)
        return o, None, ls

    Q4, K4, V4 = view4(q, Nq, qs), view4(k, Nk, ks), view4(v, Nk, vs)
    qsel = torch.tensor(sorted(set(range(max(0, Nq - 128), Nq)) | set(range(min(32, Nq))) |
                               set(int(i) for i in torch.randint(0, Nq, (256,), generator=gen))), dtype=torch.long)
    pairs = sorted({(0, 0), (B - 1, H - 1), (int(torch.randint(0, B, (1,), generator=gen)), int(torch.randint(0, H, (1,), generator=gen))),
                    (int(torch.randint(0, B, (1,), generator=gen)), int(torch.randint(0, H, (1,), generator=gen)))})
    refs, bnds = [], []
    lrefs, lbnds = [[], []], [[], []]     # log-sum-exp per segment (see "Bound, log-sum-exp" in the module docstring)
    for bb, hh in pairs:
        qq = Q4[bb, hh, qsel]
        bh = bb * H + hh
        bias = (relh[bh, qsel].to(F64), relw[bh, qsel].to(F64)) if rel else None
        s1 = attn_segment_ref(qq, K4[bb, hh], V4[bb, hh], scale, bias=bias)
        lrefs[0].append(s1["L2"])
        lbnds[0].append(s1["L2_bnd"])
        r, sv = s1["r"], s1["sv"]
        if nk2:
            K2 = k2.as_strided((B, H, nk2, D), st2 + (1,), 0).to(F64)
            V2 = k2.as_strided((B, H, nk2, D), st2 + (1,), C).to(F64)
            seg2 = attn_segment_ref(qq, K2[bb, hh], V2[bb, hh], scale)
            lrefs[1].append(seg2["L2"])
            lbnds[1].append(seg2["L2_bnd"])
            r = r + float(s2[bb]) * seg2["r"]
            sv = sv + float(s2[bb]) * seg2["sv"]
        refs.append(r)
        bnds.append(attn_out_bound(r, sv, s1["bmax"]))

    def gather(o):
        ov = o.view.reshape(B, Nq, H, D).cpu()
        return torch.cat([ov[bb, qsel, hh] for bb, hh in pairs])

    def gather_lse(ls):
        lv = ls.view.reshape(B, H, Nq).cpu()
        return torch.cat([lv[bb, hh, qsel] for bb, hh in pairs])[:, None]

    lse = [dict(name=n, ref=torch.cat(lrefs[i])[:, None], bnd=torch.cat(lbnds[i])[:, None]) for i, n in enumerate(("lse", "lse2")[:2 if nk2 else 1])]
    return dict(launch=launch, ref=torch.cat(refs), bnd=torch.cat(bnds), gather=gather, cs=False, conv=False, f32=False,
                lse=lse, gather_lse=gather_lse)


# --------------------------------------------------------------------------------------------------- the library's report of its plan
def plan_check(spec, keys):
    """the library's report of the launch (spec["plan"]) against the kernels that ran: the full gemm_kernel key, the split-K reduce, the split
    factor, the stand-alone column-statistics kernel"""
    if "plan" not in spec:
        return "n/a"
    p = spec["plan"]()
    if p is None:
        raise CaseFailure("the plan query refuses a launch that ran")
    b = ("false", "true")
    want = [] if p.rowpanel else [f"gemm_kernel<{p.BM}, {p.BN}, {p.AMODE}, {p.WAVES_M}, {p.WAVES_N}, {b[p.GLDS]}, {p.WAVES_K}, {p.STAGES}, {b[p.CS]}, {p.LAB}, {p.WA}, {p.XE}>"]
    ran = sorted(set(k for k in keys if k.startswith("gemm_kernel<")))
    problems = []
    if ran != want:
        problems.append(f"the plan says {want}, {ran} ran")
    reduced, stats = "splitk_reduce_kernel" in keys, "colstats_kernel" in keys
    if (p.splitk > 1) != reduced or bool(p.reduce) != reduced:
        problems.append(f"plan split {p.splitk} (reduce {p.reduce}) but split-K reduce {'ran' if reduced else 'did not run'}")
    if p.splitk != spec.get("ws_split", 1):
        problems.append(f"the plan splits {p.splitk} ways, the workspace is sized for {spec.get('ws_split', 1)}")
    if bool(p.colstats) != stats:
        problems.append(f"plan colstats {p.colstats} but the stand-alone colstats_kernel {'ran' if stats else 'did not run'}")
    if problems:
        raise CaseFailure("; ".join(problems))
    return "ok"


# --------------------------------------------------------------------------------------------------- driver
def run_case(c, ops):
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    op = c["op"]
    spec = (run_conv(c, ops, gen) if op == "conv" else run_up2(c, ops, gen) if op == "up2" else run_gemm(c, ops, gen, ln=(op == "ln"))
            if op in ("gemm", "ln") else run_attn(c, ops, gen))
    (o1, st1, *ex1), names = profiled(spec["launch"])
    ex1 = ex1[0] if ex1 else []          # attention: the guarded log-sum-exp buffers
    names, keys = route_keys(names)
    res = dict(id=c["id"], kernels=names, keys=sorted(set(keys)), ok=False, ratio=None, guards=None, plan=None, error=None)
    if "lse" in spec:
        res["lse_ratio"] = None
    try:
        want = RC.expected_kernels(c["id"])
        missing = [k for k in want if k not in keys]
        if missing:
            raise CaseFailure(f"declared instantiation(s) not reached: {missing}")
        res["plan"] = plan_check(spec, keys)
        o2, st2, *ex2 = spec["launch"]()
        ex2 = ex2[0] if ex2 else []
        torch.cuda.synchronize()
        gd = o1.guards_intact() and o2.guards_intact() and all(s.guards_intact() for s in [st1, st2] + ex1 + ex2 if s is not None)
        res["guards"] = "intact" if gd else "CLOBBERED"
        if not gd:
            raise CaseFailure("a guard area was written")
        if not torch.equal(o1.bits(), o2.bits()) or (st1 is not None and not torch.equal(st1.bits(), st2.bits())):
            raise CaseFailure("two runs differ")
        for info, a, b in zip(spec.get("lse", []), ex1, ex2):
            if not torch.equal(a.bits(), b.bits()):
                raise CaseFailure(f"{info['name']}: two runs differ")
            unwritten = int((a.bits() == a.sent).sum())
            if unwritten:
                raise CaseFailure(f"{info['name']}: {unwritten} of {a.cols} (batch, head, query) entries were never written")
        if "gather" in spec:
            got = spec["gather"](o1)
        else:
            got = o1.view[spec["rows"].cuda()].float().cpu() if not spec["f32"] else o1.view[spec["rows"].cuda()].cpu()
        try:
            ratio = bound_check(got, spec["ref"], spec["bnd"], "output")
        except CaseFailure as e:
            if "rows" not in spec:
                raise
            bad = ((got.to(F64) - spec["ref"]).abs() > spec["bnd"]).any(1)
            g = spec["rows"][bad]
            raise CaseFailure(f"{e}; {int(bad.sum())} of {len(bad)} checked rows fail, output rows {g[:6].tolist()} .. {g[-3:].tolist()}")
        if st1 is not None:
            y = o1.view.cpu()
            if spec.get("rs"):
                ratio = max(ratio, stats_check(st1.view.cpu(), y, 64, "row statistics", per_row=True))
            else:
                ratio = max(ratio, stats_check(st1.view.cpu(), y, 32, "column statistics", sample_rows=spec.get("sample_rows", 0)))
        if "lse" in spec:
            got_l = [spec["gather_lse"](a) for a in ex1]
            res["lse_ratio"] = max(float(((g.to(F64) - info["ref"]).abs() / info["bnd"]).nan_to_num(float("inf")).max()) for info, g in zip(spec["lse"], got_l))
            for info, g in zip(spec["lse"], got_l):
                bound_check(g, info["ref"], info["bnd"], info["name"])
        res["ratio"], res["ok"] = ratio, True
    except CaseFailure as e:
        res["error"] = str(e)
    return res


def main():
    stray = sorted(k for k in os.environ if k.startswith("AE_") and k != "AE_LIB_PATH")
    if stray:
        print(f"route_check: routing variables set: {stray} — the route cases run on the default plans only", flush=True)
        sys.exit(2)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from anyedit_amd import ops
    flt = sys.argv[1:]
    cases = [c for c in RC.CASES if not flt or any(f in c["id"] for f in flt)]
    results, t0 = [], time.time()
    aborted = None
    for c in cases:
        t1 = time.time()
        try:
            r = run_case(c, ops)
        except Exception as e:   # a HIP / runtime error: start no further GPU work
            aborted = dict(id=c["id"], error=f"{type(e).__name__}: {e}")
            print(f"ABORT {c['id']}: {aborted['error']}", flush=True)
            break
        results.append(r)
        rt = f"{r['ratio']:.3f}" if r["ratio"] is not None else "-"
        if "lse_ratio" in r:
            rt += " lse_ratio " + (f"{r['lse_ratio']:.3f}" if r["lse_ratio"] is not None else "-")
        print(f"{'PASS' if r['ok'] else 'FAIL'} {r['id']:24s} {time.time() - t1:5.1f}s ratio {rt:>6s} guards {r['guards']} plan {r['plan']} "
              f"kernels {r['keys'] or r['kernels']}" + (f"  ERROR {r['error']}" if r["error"] else ""), flush=True)
    summary = dict(results=results, aborted=aborted, seconds=round(time.time() - t0, 1))
    print("ROUTE_SUMMARY " + json.dumps(summary), flush=True)
    sys.exit(0 if aborted is None and all(r["ok"] for r in results) else 1)


if __name__ == "__main__":
    main()
