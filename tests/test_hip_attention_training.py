"""GPU tests of the attention forward (with its log-sum-exp outputs) and ae_attn_bwd_bf16 in the layouts the training step uses, against
the float64 formulas of tests/attn_ref.py on the same bf16-rounded operands.

Layouts (B = 2, H = 3 unless a case says otherwise: B != H, H not a power of two, so a (batch, head) mix-up cannot cancel):
  qkv   fused rows [B*N, 3C + 8], head stride D; the gradients go into a fused buffer of the same shape;
  q_kv  query rows [B*Nq, C + 8] and packed key/value rows [B*Nk, 2C + 8];
  bhnd  [B, H, n, D + 8] per operand.
Every row is 8 elements wider than its logical content.  Inputs keep a NaN sentinel in that pad (a read of it poisons the result); every
output (out, lse, lse2, delta, dq, dk, dv) is a view of a sentinel-filled allocation with guard bands before and after: after each call
everything outside the logical views must be unchanged and everything inside finite and written, and a second call on fresh buffers must
be bit-identical.  (lse, lse2 and delta are dense [B, H, Nq] by the C ABI: guard bands only, no row pad.)

Comparison per (batch, head) slice, with the tolerances of test_hip_backward.py::test_attention_backward (relative L2 / max-abs over max):
lse 2e-3 / 5e-3, delta 2e-2 / 5e-2, dV 1e-2 / 3e-2, dK and dQ 1.5e-2 / 5e-2, the forward output 6e-3 / 3e-2.

Every comparison of a test is made and printed before the test fails, so one run shows all its figures.

Four comparisons are not the plain ones, each with its derivation:
  * peaked softmax (q x 6) at head dim 40, gradients: ae_attn_bwd_bf16 does not normalise, it takes P = 2^(c2 s - L2) from the L2 it is handed.
    The forward of head dim 40 rounds scale log2(e) q to bf16 (next item), so its L2 is off by up to 2^-9 of the logit's absolute products —
    measured 1e-3 .. 1.5e-3 of |L2| ~ 30, i.e. e ~ 0.02 .. 0.05 — and every probability of a row by the factor 2^-e: to first order
    dQ~ - dQ = e ln2 (-dQ + g scale delta (P K)), and in the one-hot regime dQ is a small difference while delta P K is not.  Measured
    against the exact formulas: dQ rel-L2 2.3e-2 (2e-2 asked) at head dim 40, 5.8e-3 at head dim 64, whose forward keeps fp32 logits and
    an lse within 1e-7.  So at head dim 40 the backward is compared with the float64 formulas AT THE LSE IT WAS HANDED
    (attn_ref.segment(given_lse=...), and given_delta = rowsum(dO o out) for the call that takes delta from the output), with the same
    2e-2 / 6e-2; the lse itself is compared with the exact one at its own tolerance, and the figures against the exact formulas are printed.
  * Nk = 1, lse: the log-sum-exp of one key is the logit itself, scale q.k, which cancels to anything between 0 and sum_d |q_d k_d|, and
    no sum over keys averages a rounding out.  The forward kernels of head dims 40 / 80 / 160 (attention_fast.hip) round scale log2(e) q
    to bf16 once for the logit MFMA: 2^-9 relative per product, i.e. up to 2^-9 scale sum_d |q_d| |k_d| per logit, which is 2 - 3e-3 of
    the rms logit over a slice and unbounded relative to a single logit (Nq = Nk = 1).  These cases take the element-wise bound of
    tools/route_check.py instead:  |got - L2| <= log2(e) (2^-8 + (2^-9 + 2^-16) scale sum_d |q_d| |k_d|) + 2^-22 |L2| + 1e-6
    (bf16 denominator, bf16 pre-scaled Q + fp32 accumulation, fp32 store).  A wrong row, head or batch is off by the logits' spread, O(1).
  * Nk = 1, dQ and dK: P = 1, so dS = P o (dP - delta) = 0 and the true dQ, dK are exactly zero — a relative tolerance has no meaning.
    The kernel forms dS from bf16 operands: T1 - delta T2 with T1 = bf16(P o dP) K, T2 = bf16(P) K (or bf16(P o (dP - delta)) with the
    forward output at hand), each rounding within 2^-9 of |dP|: 2^-8, doubled for the fp32 exp2 / accumulation.  And its P is 2^(c2 s - L2)
    from the L2 it is handed, whose error e_q (natural units; bounded in the next item) leaves P = 1 - e_q and dS = P (1 - P) dP ~ e_q dP.
    With k_q = 2^-7 + 2^-8 + (2^-9 + 2^-16) scale sum_d |q_d| |k_d| and |dP_q| <= A_q = sum_d |dO_qd| |v_d|:
        |dQ_qd| <= g scale k_q A_q |k_d|,        |dK_d| <= g scale sum_q k_q A_q |Q_qd|.
    Where such a call ADDS onto an existing dQ (the second segment of the two-segment case), the sum is compared with the first
    segment's dQ at the usual tolerance after each element's difference has been reduced by that bound.
  * the gate gradient sum_{h, q} delta[b] against float64: the delta errors of different rows are independent roundings (bf16 P, the
    forward's lse), so they add in quadrature: |sum got - sum ref| <= 3 * 2e-2 * ||delta_ref[b]||_2 (three standard deviations of a sum
    whose terms meet the delta tolerance); a systematic error (a gate factor in delta, a dropped head) is of the order ||delta_ref[b]||_1.
"""
import contextlib
import functools
import zlib

import pytest
import torch

import attn_ref as R
from conftest import rel_l2

gpu = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
SENT = {BF: 0x7FA5, F32: 0x7FA5A5A5}      # NaN bit patterns no kernel writes
GUARD = 4096
PAD = 8
TOL = dict(lse=(2e-3, 5e-3), delta=(2e-2, 5e-2), dv=(1e-2, 3e-2), dk=(1.5e-2, 5e-2), dq=(1.5e-2, 5e-2), out=(6e-3, 3e-2))
PEAKED = dict({k: (2e-2, 6e-2) for k in TOL}, lse=TOL["lse"])   # test_attention_fuzz's tolerances: the peaked-softmax case only
FAST_D = (40, 64, 80, 160)


@pytest.fixture(scope="module")
def ops():
    from anyedit_amd import ops as o
    return o


# --------------------------------------------------------------------------------------------------- guarded buffers
class Buf:
    """`n` elements between two guard bands, all sentinel-filled; `view` registers a logical (strided) view of it."""

    def __init__(self, n, dtype=BF):
        self.raw = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.iv = self.raw.view(torch.int16 if dtype == BF else torch.int32)
        self.sent = SENT[dtype]
        self.iv.fill_(self.sent)
        self.logical = torch.zeros(n + 2 * GUARD, dtype=torch.bool, device=DEV)

    def at(self, off=0):
        return self.raw[GUARD + off:]

    def view(self, shape, strides, off=0):
        idx = torch.arange(self.raw.numel(), device=DEV).as_strided(shape, strides, GUARD + off)
        self.logical[idx.reshape(-1)] = True
        return self.raw.as_strided(shape, strides, GUARD + off)

    def check(self, what, written=True):
        stray = int((self.iv[~self.logical] != self.sent).sum())
        assert stray == 0, f"{what}: {stray} elements outside the logical view were written"
        inside = self.iv[self.logical]
        if written:
            left = int((inside == self.sent).sum())
            assert left == 0, f"{what}: {left} of {inside.numel()} elements were never written"
            assert bool(torch.isfinite(self.raw[self.logical].float()).all()), f"{what}: non-finite values"
        else:
            assert bool((inside == self.sent).all()), f"{what}: written although no gradient was asked for"


class Op:
    """One (B, H, n, D) operand inside a Buf: element offset + (batch, head, row) strides."""

    def __init__(self, buf, off, strides, shape):
        self.buf, self.off, self.st = buf, off, tuple(strides)
        self.v4 = buf.view(shape, self.st + (1,), off)

    @property
    def ptr(self):
        return self.buf.at(self.off)

    def cpu(self):
        return self.v4.float().cpu()


def geometry(lay, B, H, Nq, Nk, D):
    """name -> (buffer key, element offset, strides, rows); buffer key -> elements"""
    C = H * D
    if lay == "qkv":
        assert Nq == Nk
        ld = 3 * C + PAD
        st = (Nq * ld, D, ld)
        return dict(q=("a", 0, st, Nq), k=("a", C, st, Nk), v=("a", 2 * C, st, Nk)), dict(a=B * Nq * ld)
    if lay == "q_kv":
        lq, lk = C + PAD, 2 * C + PAD
        sk = (Nk * lk, D, lk)
        return dict(q=("a", 0, (Nq * lq, D, lq), Nq), k=("b", 0, sk, Nk), v=("b", C, sk, Nk)), dict(a=B * Nq * lq, b=B * Nk * lk)
    ld = D + PAD
    sq, sk = (H * Nq * ld, Nq * ld, ld), (H * Nk * ld, Nk * ld, ld)
    return dict(q=("a", 0, sq, Nq), k=("b", 0, sk, Nk), v=("c", 0, sk, Nk)), dict(a=B * H * Nq * ld, b=B * H * Nk * ld, c=B * H * Nk * ld)


def alloc(geo, sizes, B, H, D):
    bufs = {key: Buf(n) for key, n in sizes.items()}
    return bufs, {name: Op(bufs[key], off, st, (B, H, n, D)) for name, (key, off, st, n) in geo.items()}


def twice(launch):
    """launch() -> {name: (Buf, written)} on fresh buffers.  Runs it twice: every buffer intact outside / written inside, the two runs
    bit-identical.  Returns the first run's dict."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    for r in (a, b):
        seen = set()
        for name, (buf, written) in r.items():
            if id(buf) not in seen:
                seen.add(id(buf))
                buf.check(name, written)
    for name in a:
        assert torch.equal(a[name][0].iv, b[name][0].iv), f"{name}: two runs differ"
    return a


# --------------------------------------------------------------------------------------------------- comparison
_MISSES = []   # value comparisons that missed, of the test that is running: all of them are made (and printed) before the test fails


def collects(test):
    @functools.wraps(test)
    def run(*a, **kw):
        _MISSES.clear()
        test(*a, **kw)
        assert not _MISSES, f"{len(_MISSES)} comparison(s) missed:\n  " + "\n  ".join(_MISSES)
    return run


_INFO = [False]


@contextlib.contextmanager
def informational():
    """comparisons inside are printed, not asserted"""
    _INFO[0] = True
    try:
        yield
    finally:
        _INFO[0] = False


def expect(ok, msg):
    print(("info  " if _INFO[0] else "ok    " if ok else "MISS  ") + msg)
    if not ok and not _INFO[0]:
        _MISSES.append(msg)


def close(got, ref, rl2, mabs, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e = rel_l2(got, ref)
    m = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
    expect(e <= rl2 and m <= mabs, f"{what}: rel_l2={e:.3e} (<= {rl2}), max_abs/max={m:.3e} (<= {mabs})")


def per_slice(kind, got, ref, what, tol=TOL):
    """got / ref [B, H, ...]: every (batch, head) slice on its own, so one wrong head is not diluted"""
    got = got.float().cpu() if got.is_cuda else got
    for b in range(ref.shape[0]):
        for h in range(ref.shape[1]):
            close(got[b, h], ref[b, h], *tol[kind], what=f"{what} {kind}[b={b}, h={h}]")


def zero_bounded(got, bnd, what):
    """a gradient whose true value is exactly zero (Nk = 1): element-wise absolute bound, see the module docstring"""
    got = got.float().cpu().to(F64)
    ratio = float((got.abs() / (bnd + 1e-30)).max())
    expect(ratio <= 1.0, f"{what}: true value 0, max |got| / rounding bound = {ratio:.3f} (<= 1)")


def gate_gradient(delta, ref_delta, what):
    got = delta.float().cpu().to(F64).sum((1, 2))
    ref = ref_delta.sum((1, 2))
    lim = 3 * TOL["delta"][0] * ref_delta.flatten(1).norm(dim=1)
    expect(bool(((got - ref).abs() <= lim).all()), f"{what}: gate gradient {got.tolist()} vs {ref.tolist()} (allowed difference {lim.tolist()})")


def compare_lse(P, got, ref_lse, what, tol=TOL, Nk=None, kcpu="k"):
    if (Nk or P.Nk) > 1:
        return per_slice("lse", got, ref_lse, what, tol)
    # one key: element-wise bound (module docstring)
    qk = (P.cpu["q"].abs() @ P.cpu[kcpu].abs().transpose(-1, -2))[..., 0]
    bnd = R.LOG2E * (2.0 ** -8 + (2.0 ** -9 + 2.0 ** -16) * P.scale * qk) + 2.0 ** -22 * ref_lse.abs() + 1e-6
    ratio = float(((got.float().cpu().to(F64) - ref_lse).abs() / bnd).max())
    expect(ratio <= 1.0, f"{what} lse (one key): max |got - ref| / bound = {ratio:.3f} (<= 1)")


# --------------------------------------------------------------------------------------------------- one attention problem
class Problem:
    def __init__(self, lay, B, H, Nq, Nk, D, q_gain=1.0, tag=""):
        self.lay, self.B, self.H, self.Nq, self.Nk, self.D, self.C = lay, B, H, Nq, Nk, D, H * D
        self.scale = D ** -0.5
        gen = self.gen = torch.Generator().manual_seed(zlib.crc32(repr((lay, B, H, Nq, Nk, D, tag)).encode()))
        self.geo, self.sizes = geometry(lay, B, H, Nq, Nk, D)
        self.in_bufs, self.x = alloc(self.geo, self.sizes, B, H, D)
        self.cpu = {}
        for name, gain in (("q", q_gain), ("k", 1.0), ("v", 1.0)):
            self.cpu[name] = self._fill(self.x[name], gain)
        lo = self.C + PAD
        self.o_geo = dict(o=("o", 0, (Nq * lo, D, lo), Nq)), dict(o=B * Nq * lo)
        _, d = alloc(*self.o_geo, B, H, D)
        self.dO = d["o"]
        self.cpu["dO"] = self._fill(self.dO)

    def _fill(self, op, gain=1.0):
        t = (torch.randn(op.v4.shape, generator=self.gen) * gain).to(BF)
        op.v4.copy_(t)
        return t.to(F64)

    def ref(self, gate=None, k="k", v="v"):
        return R.segment(self.cpu["q"], self.cpu[k], self.cpu[v], self.scale, self.cpu["dO"], gate=gate)

    def stat(self):
        B, H, Nq = self.B, self.H, self.Nq
        buf = Buf(B * H * Nq, F32)
        return buf, buf.view((B, H, Nq), (H * Nq, Nq, 1))

    def new_out(self, prev=None):
        _, d = alloc(*self.o_geo, self.B, self.H, self.D)
        if prev is not None:
            d["o"].v4.copy_(prev)
        return d["o"]

    def forward(self, ops, seg2=None, out_scale=None, onto=None, want_lse=True, kv=None, Nk=None):
        """-> launch function for `twice`; seg2 = (k2 Op, v2 Op, Nk2, gate tensor); onto: bf16 [B, H, Nq, D] to accumulate onto;
        kv / Nk: another key/value segment in place of this problem's own"""
        B, H, Nq, D = self.B, self.H, self.Nq, self.D
        Nk = Nk or self.Nk
        x = dict(self.x, k=kv["k"], v=kv["v"]) if kv is not None else self.x

        def launch():
            o = self.new_out(onto)
            res = dict(out=(o.buf, True))
            kw = {}
            if want_lse:
                lb, lv = self.stat()
                res["lse"] = (lb, True)
                kw["lse"] = lv
            if seg2 is not None:
                k2, v2, Nk2, gate = seg2
                kw["seg2"] = (k2.ptr, v2.ptr, Nk2, k2.st, v2.st, gate)
                if want_lse:
                    lb2, lv2 = self.stat()
                    res["lse2"] = (lb2, True)
                    kw["lse2"] = lv2
            ops.attention(x["q"].ptr, x["k"].ptr, x["v"].ptr, B, H, Nq, Nk, D, self.scale, x["q"].st, x["k"].st, x["v"].st, out=o.ptr,
                          o_strides=o.st, out_scale=out_scale, accumulate=onto is not None, **kw)
            self._last = dict(out=o, lse=kw.get("lse"), lse2=kw.get("lse2"))
            return res

        return launch

    def run_forward(self, ops, **kw):
        """runs the forward twice; returns the FIRST run's (out Op, lse view, lse2 view)"""
        keep = []

        def launch():
            r = self.forward(ops, **kw)()
            keep.append(self._last)
            return r

        twice(launch)
        return keep[0]

    def backward(self, ops, lse, k="k", v="v", Nk=None, kv=None, gate=None, dq_prev=None, out=None, want_kv=True, split=True, accumulate=False):
        """runs ae_attn_bwd_bf16 twice on fresh gradient buffers; returns the first run's dict(dq, dk, dv Ops, delta view).  kv: Ops of another
        key/value segment (with geometry kv_geo); dq_prev: bf16 [B, H, Nq, D] the dQ pass adds onto."""
        B, H, Nq, D = self.B, self.H, self.Nq, self.D
        x = dict(self.x)
        geo, sizes = self.geo, self.sizes
        if kv is not None:
            x["k"], x["v"], geo, sizes = kv["k"], kv["v"], kv["geo"], kv["sizes"]
        Nk = Nk or self.Nk
        keep = []

        def launch():
            if kv is None:
                gb, g = alloc(geo, sizes, B, H, D)
            else:   # the query gradient in this problem's own geometry, the key/value gradients in the segment's
                gb, g = alloc(self.geo, self.sizes, B, H, D)
                gb2, g2 = alloc(geo, sizes, B, H, D)
                g["k"], g["v"] = g2["k"], g2["v"]
            if dq_prev is not None:
                g["q"].v4.copy_(dq_prev)
            db, dv_ = self.stat()
            delta = ops.attention_bwd(x["q"].ptr, x["k"].ptr, x["v"].ptr, self.dO.ptr, lse, B, H, Nq, Nk, D, self.scale, x["q"].st, x["k"].st,
                                      x["v"].st, g["q"].ptr, g["k"].ptr if want_kv else None, g["v"].ptr if want_kv else None, g["q"].st,
                                      g["k"].st, g["v"].st, out_scale=gate, accumulate_dq=accumulate, out=out.ptr if out is not None else None,
                                      split_dkv=split, o_strides=self.dO.st, delta=dv_)
            assert delta.data_ptr() == dv_.data_ptr()
            keep.append(dict(dq=g["q"], dk=g["k"], dv=g["v"], delta=dv_))
            res = dict(delta=(db, True))
            shared = g["q"].buf is g["k"].buf                       # fused qkv: one buffer, written only where a gradient was asked for
            if shared:
                if want_kv:
                    res["dqkv"] = (g["q"].buf, True)
                else:                                               # the k / v thirds must keep the sentinel: checked by the caller
                    res["dqkv"] = (g["q"].buf, None)
            else:
                res["dq"] = (g["q"].buf, True)
                for name in ("k", "v"):
                    res["d" + name] = (g[name].buf, want_kv)
            return res

        def checked():
            r = launch()
            return {n: (b, w) for n, (b, w) in r.items() if w is not None}

        twice(checked)
        return keep[0]


def compare_backward(P, got, ref, what, gate=None, tol=TOL, dq_ref=None, Nk=None, kcpu="k", vcpu="v", want_kv=True, dq=True):
    """got: Problem.backward's dict; ref: attn_ref.segment's.  dq_ref: what the query gradient buffer should hold when the call accumulates."""
    Nk = Nk or P.Nk
    per_slice("delta", got["delta"], ref["delta"], what, tol)
    g = torch.ones(P.B, dtype=F64) if gate is None else gate.cpu().to(F64)
    if Nk == 1:   # true dQ, dK are zero: the rounding bound of the module docstring
        A = P.cpu["dO"].abs() @ P.cpu[vcpu].abs().transpose(-1, -2)                                  # [B, H, Nq, 1]: |dO_q| . |v|
        kq = 2.0 ** -7 + 2.0 ** -8 + (2.0 ** -9 + 2.0 ** -16) * P.scale * (P.cpu["q"].abs() @ P.cpu[kcpu].abs().transpose(-1, -2))
        c = P.scale * g[:, None, None, None]
        assert float(ref["dq"].abs().max()) <= 1e-12 and float(ref["dk"].abs().max()) <= 1e-12
        dq_bound = c * kq * A * P.cpu[kcpu].abs()
        if dq and dq_ref is None:
            zero_bounded(got["dq"].v4, dq_bound, what + " dq")
        if want_kv:
            zero_bounded(got["dk"].v4, c * ((kq * A).transpose(-1, -2) @ P.cpu["q"].abs()), what + " dk")
        if dq and dq_ref is not None:
            err = got["dq"].v4.float().cpu().to(F64) - dq_ref
            reduced = dq_ref + err.sign() * (err.abs() - dq_bound).clamp_min(0)
            per_slice("dq", reduced, dq_ref, what + " (accumulated, less the one-key rounding bound)", tol)
            dq = False
    else:
        if dq and dq_ref is None:
            per_slice("dq", got["dq"].v4, ref["dq"], what, tol)
        if want_kv:
            per_slice("dk", got["dk"].v4, ref["dk"], what, tol)
    if dq and dq_ref is not None:
        per_slice("dq", got["dq"].v4, dq_ref, what + " (accumulated)", tol)
    if want_kv:
        per_slice("dv", got["dv"].v4, ref["dv"], what, tol)


def forward_and_backward(ops, P, what, tol=TOL, at_given_lse=False):
    """forward with lse, backward without and with the forward output (PRE); all against float64.  at_given_lse: the gradients against
    the formulas evaluated at the lse (and output) the backward was handed — see the module docstring."""
    ref = P.ref()
    f = P.run_forward(ops)
    per_slice("out", f["out"].v4, ref["out"], what, tol)
    compare_lse(P, f["lse"], ref["lse"], what, tol)
    b1 = P.backward(ops, f["lse"])
    b2 = P.backward(ops, f["lse"], out=f["out"])
    if not at_given_lse:
        compare_backward(P, b1, ref, what, tol=tol)
        compare_backward(P, b2, ref, what + " (delta from the output)", tol=tol)
        return
    with informational():
        compare_backward(P, b1, ref, what + " [exact formulas]", tol=tol)
        compare_backward(P, b2, ref, what + " [exact formulas] (delta from the output)", tol=tol)
    lse = f["lse"].cpu().to(F64)
    compare_backward(P, b1, R.segment(P.cpu["q"], P.cpu["k"], P.cpu["v"], P.scale, P.cpu["dO"], given_lse=lse), what + " at the given lse", tol=tol)
    per_slice("delta", b2["delta"], ref["delta"], what + " (delta from the output)", tol)
    d_out = (P.cpu["dO"] * f["out"].v4.cpu().to(F64)).sum(-1)
    ref2 = R.segment(P.cpu["q"], P.cpu["k"], P.cpu["v"], P.scale, P.cpu["dO"], given_lse=lse, given_delta=d_out)
    compare_backward(P, b2, ref2, what + " at the given lse (delta from the output)", tol=tol)


# --------------------------------------------------------------------------------------------------- cases
@gpu
@pytest.mark.parametrize("lay,Nq,Nk", [("q_kv", 130, 77), ("qkv", 200, 200)])
@pytest.mark.parametrize("D", [8, 16, 32, 40, 48, 64, 80, 96, 128, 160])
@collects
def test_every_instantiated_head_dim(ops, D, lay, Nq, Nk):
    forward_and_backward(ops, Problem(lay, 2, 3, Nq, Nk, D), f"D={D} {lay} {Nq}x{Nk}")


@gpu
@pytest.mark.parametrize("Nq,Nk", [(1, 1), (65, 1), (33, 65), (129, 4)])
@pytest.mark.parametrize("D", FAST_D)
@collects
def test_edges(ops, D, Nq, Nk):
    forward_and_backward(ops, Problem("bhnd", 2, 3, Nq, Nk, D), f"D={D} bhnd {Nq}x{Nk}")


def _gate():
    return torch.tensor([0.7, 1.3], dtype=F32, device=DEV)


@gpu
@pytest.mark.parametrize("D", FAST_D)
@collects
def test_gate_scales_the_gradients_and_leaves_delta_alone(ops, D):
    P = Problem("q_kv", 2, 3, 130, 77, D)
    gate = _gate()
    ref = P.ref(gate=gate.cpu())
    what = f"D={D} gated"
    f = P.run_forward(ops, out_scale=gate)
    per_slice("out", f["out"].v4, gate.cpu().to(F64)[:, None, None, None] * ref["out"], what)
    per_slice("lse", f["lse"], ref["lse"], what)                      # independent of out_scale
    b = P.backward(ops, f["lse"], gate=gate)
    compare_backward(P, b, ref, what, gate=gate)                      # ref["delta"] is un-scaled
    gate_gradient(b["delta"], ref["delta"], what)
    # the forward output handed over with a gate is not this segment's alone: the call must not take delta from it
    b2 = P.backward(ops, f["lse"], gate=gate, out=f["out"])
    compare_backward(P, b2, ref, what + " (out= ignored)", gate=gate)


@gpu
@pytest.mark.parametrize("D", FAST_D)
@collects
def test_accumulate_dq_adds_onto_an_existing_gradient(ops, D):
    P = Problem("q_kv", 2, 3, 130, 77, D)
    gate = _gate()
    ref = P.ref(gate=gate.cpu())
    f = P.run_forward(ops)
    rms = float(ref["dq"].pow(2).mean().sqrt())
    prev = (torch.randn(ref["dq"].shape, generator=P.gen) * rms).to(BF)
    b = P.backward(ops, f["lse"], gate=gate, dq_prev=prev, accumulate=True)
    compare_backward(P, b, ref, f"D={D} dq +=", gate=gate, dq_ref=prev.to(F64) + ref["dq"])


@gpu
@pytest.mark.parametrize("lay,Nq,Nk", [("q_kv", 130, 77), ("qkv", 200, 200)])
@pytest.mark.parametrize("D", FAST_D)
@collects
def test_dq_only_leaves_the_key_value_gradients_untouched(ops, D, lay, Nq, Nk):
    P = Problem(lay, 2, 3, Nq, Nk, D)
    ref = P.ref()
    f = P.run_forward(ops)
    full = P.backward(ops, f["lse"])
    only = P.backward(ops, f["lse"], want_kv=False)
    what = f"D={D} {lay} dq only"
    compare_backward(P, only, ref, what, want_kv=False)
    assert torch.equal(only["dq"].v4, full["dq"].v4) and torch.equal(only["delta"], full["delta"]), "dQ / delta depend on whether dK / dV were asked for"
    for name in ("dk", "dv"):                                         # (separate buffers were checked whole; fused rows: the k / v thirds and the pad)
        op = only[name]
        bits = op.v4.contiguous().view(torch.int16)
        assert bool((bits == SENT[BF]).all()), f"{what}: {name} was written"
    if lay == "qkv":
        buf = only["dq"].buf
        keep = torch.zeros_like(buf.logical)
        idx = torch.arange(buf.raw.numel(), device=DEV).as_strided(only["dq"].v4.shape, only["dq"].v4.stride(), GUARD + only["dq"].off)
        keep[idx.reshape(-1)] = True
        assert bool((buf.iv[~keep] == buf.sent).all()), f"{what}: the fused gradient buffer was written outside its q third"
        assert not bool((buf.iv[keep] == buf.sent).any()), f"{what}: dq left unwritten"


@gpu
@pytest.mark.parametrize("D", [40, 80, 160])
@collects
def test_split_key_pass_writes_through_strides(ops, D):
    """B H = 2 blocks against 9 query tiles: four splits, the last one empty; H = 2 and packed key/value rows, so attn_bwd_reduce_kernel's
    (batch, head, row) strides matter."""
    from anyedit_amd._lib import lib
    B, H, Nq, Nk = 1, 2, 520, 78
    assert lib.ae_attn_bwd_workspace_floats(B, H, Nq, Nk, D) == 4 * B * H * Nk * 2 * ((D + 15) // 16 * 16)
    P = Problem("q_kv", B, H, Nq, Nk, D)
    ref = P.ref()
    f = P.run_forward(ops)
    what = f"D={D} split"
    per_slice("lse", f["lse"], ref["lse"], what)
    split = P.backward(ops, f["lse"], split=True)
    compare_backward(P, split, ref, what)
    whole = P.backward(ops, f["lse"], split=False)
    compare_backward(P, whole, ref, what + " (one block)")
    assert torch.equal(split["dq"].v4, whole["dq"].v4)
    for name in ("dk", "dv"):
        sp, wh = split[name].cpu(), whole[name].cpu()
        for h in range(H):
            close(sp[0, h], wh[0, h], 2e-3, 8e-3, f"{what} {name}[h={h}] vs one block")


def _second_segment(P, Nk2):
    B, H, D, C = P.B, P.H, P.D, P.C
    lk = 2 * C + PAD
    st = (Nk2 * lk, D, lk)
    geo, sizes = dict(k=("b", 0, st, Nk2), v=("b", C, st, Nk2)), dict(b=B * Nk2 * lk)
    _, d = alloc(geo, sizes, B, H, D)
    P.cpu["k2"], P.cpu["v2"] = P._fill(d["k"]), P._fill(d["v"])
    # gradient geometry of the segment: `q` rides along so that alloc() can build all three
    ggeo = dict(geo, q=P.geo["q"])
    gsizes = dict(sizes, a=P.sizes["a"]) if P.geo["q"][0] == "a" else sizes
    return dict(k=d["k"], v=d["v"], geo=ggeo, sizes=gsizes)


@gpu
@pytest.mark.parametrize("Nk2", [1, 16])
@pytest.mark.parametrize("D", FAST_D)
@collects
def test_two_segments_as_the_tape_issues_them(ops, D, Nk2):
    P = Problem("q_kv", 2, 3, 130, 77, D, tag=f"seg2-{Nk2}")
    s2 = _second_segment(P, Nk2)
    gate = _gate()
    g64 = gate.cpu().to(F64)[:, None, None, None]
    r1, r2 = P.ref(), P.ref(gate=gate.cpu(), k="k2", v="v2")
    what = f"D={D} Nk2={Nk2}"
    f = P.run_forward(ops, seg2=(s2["k"], s2["v"], Nk2, gate))
    per_slice("out", f["out"].v4, r1["out"] + g64 * r2["out"], what)
    per_slice("lse", f["lse"], r1["lse"], what)
    compare_lse(P, f["lse2"], r2["lse"], what + " second segment", Nk=Nk2, kcpu="k2")
    b1 = P.backward(ops, f["lse"])
    compare_backward(P, b1, r1, what + " first")
    b2 = P.backward(ops, f["lse2"], kv=s2, Nk=Nk2, gate=gate, dq_prev=b1["dq"].v4, accumulate=True)
    # the first call's dQ is stored in bf16; the second adds the second segment's onto it
    compare_backward(P, b2, r2, what + " second", gate=gate, Nk=Nk2, kcpu="k2", vcpu="v2", dq_ref=r1["dq"] + r2["dq"])
    gate_gradient(b2["delta"], r2["delta"], what)


@gpu
@pytest.mark.parametrize("Nk2", [1, 16])
@pytest.mark.parametrize("D", FAST_D)
@collects
def test_unfused_forward_pair(ops, D, Nk2):
    """out = Attn(q, K, V), then out += gate * Attn(q, K2, V2) in place (the adapter form the Tape uses when it does not fuse)"""
    P = Problem("q_kv", 2, 3, 130, 77, D, tag=f"pair-{Nk2}")
    s2 = _second_segment(P, Nk2)
    gate = _gate()
    g64 = gate.cpu().to(F64)[:, None, None, None]
    r1, r2 = P.ref(), P.ref(k="k2", v="v2")
    what = f"D={D} Nk2={Nk2} pair"
    f1 = P.run_forward(ops)
    per_slice("out", f1["out"].v4, r1["out"], what + " first")
    first = f1["out"].v4.clone()
    f2 = P.run_forward(ops, out_scale=gate, onto=first, kv=s2, Nk=Nk2)
    per_slice("out", f2["out"].v4, first.float().cpu().to(F64) + g64 * r2["out"], what + " accumulated")
    compare_lse(P, f2["lse"], r2["lse"], what + " second segment", Nk=Nk2, kcpu="k2")   # independent of out_scale / accumulate


@gpu
@pytest.mark.parametrize("D", [40, 64])
@collects
def test_peaked_softmax(ops, D):
    """q x 6: logits reach tens, many rows are nearly one-hot — the lse rebase, exp2(c2 s - L2) and the delta recompute in that regime"""
    P = Problem("qkv", 2, 3, 200, 200, D, q_gain=6.0)
    forward_and_backward(ops, P, f"D={D} peaked", tol=PEAKED, at_given_lse=(D == 40))
