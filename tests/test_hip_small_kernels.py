"""Every `extern "C"` launch entry point of csrc/elementwise.hip, backward.hip, gate.hip and expert_kv.hip against tests/small_ref.py: seeded
operands, the fp32 stand-in (bit for bit) or a float64 reference with an element-wise bound, at the smallest shapes where the kernel can go
wrong — odd sizes, sizes off the vector width, the threshold between two code paths, and one case per grid-capped kernel with more work
items than one pass of its grid (small_ref.GRID_WRAP).

Every case runs twice and the two results must agree bit for bit.  Where the test owns the output (the C ABI, or a wrapper's `out=`) it is a
guarded buffer: sentinel-filled, with guard bands on both sides; nothing outside the logical view may change and everything inside must be
written.  A grid-wrap case always goes through such a buffer: a pass that is skipped leaves the sentinel (a fresh allocation could hold the
first run's result).  Rejection tests rely on checks that return before any launch.  The worst error / bound per kernel is printed when the
module finishes (`-s`), which is where DESIGN.md's table comes from."""
import collections
import math

import pytest
import torch

import small_ref as R
from small_ref import SamplerStandIns as SI

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
SENT = {BF: 0x7FA5, F32: 0x7FA5A5A5, torch.int32: 0x7FA5A5A5}      # NaN bit patterns no kernel writes
GUARD = 4096
RATIOS = collections.defaultdict(float)
COEFFS = tuple(R.c32(v) for v in (0.94, 0.3410, 0.3976, 0.9149, 0.07))


@pytest.fixture(scope="module")
def ops():
    from anyedit_amd import ops as o
    yield o
    print("\nworst error / bound per kernel (0 = bit-exact)")
    for k in sorted(RATIOS):
        print(f"  ratio {k:<34s} {RATIOS[k]:.4f}")


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a failed assertion lets the module go on; an error of the device ends it (nothing more is launched on a faulted GPU)"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit(f"GPU error, stopping: {e}", returncode=3)


def S():
    return torch.cuda.current_stream().cuda_stream


def d(t):
    return None if t is None else t.to(DEV)


def P(t):
    return None if t is None else t.data_ptr()


class Buf:
    """`shape` elements between two guard bands; sentinel-filled, or prefilled with `fill` (an accumulation target)"""

    def __init__(self, shape, dtype=BF, fill=None, ld=None):
        self.shape = tuple(shape)
        n = math.prod(self.shape) if ld is None else self.shape[0] * ld
        self.raw = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.iv = self.raw.view(torch.int16 if dtype == BF else torch.int32)
        self.sent = SENT[dtype]
        self.iv.fill_(self.sent)
        self.inside = torch.zeros(n + 2 * GUARD, dtype=torch.bool, device=DEV)
        if ld is None:
            self.t = self.raw[GUARD:GUARD + n].view(self.shape)
            self.inside[GUARD:GUARD + n] = True
        else:
            self.t = self.raw[GUARD:GUARD + n].view(self.shape[0], ld)[:, :self.shape[1]]
            self.inside[GUARD:GUARD + n].view(self.shape[0], ld)[:, :self.shape[1]] = True
        self.prefilled = fill is not None
        if fill is not None:
            self.t.copy_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def done(self, what):
        """guards intact, everything inside written -> the result on the CPU"""
        stray = int((self.iv[~self.inside] != self.sent).sum())
        assert stray == 0, f"{what}: {stray} elements outside the logical view were written"
        if not self.prefilled:
            left = int((self.iv[self.inside] == self.sent).sum())
            assert left == 0, f"{what}: {left} of {int(self.inside.sum())} elements were never written"
        return self.t.cpu().contiguous()


def twice(fn, what):
    """fn() -> a CPU tensor, None, or a tuple of them; run twice, bit-equal"""
    a, b = fn(), fn()
    la, lb = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for i, (u, v) in enumerate(zip(la, lb)):
        assert (u is None) == (v is None)
        if u is not None:
            R.check_bits(v, u, f"{what}: output {i} of the second run against the first")
    return a


def rec(name, ratio):
    RATIOS[name] = max(RATIOS[name], ratio)


def bits(name, got, ref, what=""):
    rec(name, R.check_bits(got, ref, f"{name} {what}"))


def near(name, got, ref, bnd, what=""):
    rec(name, R.check_elements(got, ref, bnd, f"{name} {what}"))


def ids(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k != "seed")


def cases(name):
    return pytest.mark.parametrize("c", R.CASES[name], ids=ids)


def rejects(ops, fn):
    """refused by a wrapper check or an AE_REQUIRE of the entry point, both of which return before any launch"""
    from anyedit_amd._lib import AnyEditHipError
    with pytest.raises((AnyEditHipError, ValueError, TypeError)):
        fn()


# ====================================================================================================== sampler kernels (bit-exact)
@cases("ae_ddim_step_f32")
def test_ddim_step(ops, c):
    g = R.gen(100 + c["branches"])
    n, br = c["n"], c["branches"]
    shape = (n,) if c.get("wrap") else (3, 4, 5, 7)
    x, eps = R.randn(g, *shape), R.randn(g, br * shape[0], *shape[1:])
    nz = R.randn(g, *shape) if c["noise"] else None
    ref = R.ref_ddim_step(x, eps, COEFFS, br, 7.5, 1.5, nz, 0.8)
    xd, ed, nd = d(x), d(eps), d(nz)

    def run():
        if c.get("wrap"):
            o = [Buf(shape, F32) for _ in range(3)]
            ops.check(ops.lib.ae_ddim_step_f32(P(xd), P(ed), P(nd), o[0].ptr, o[1].ptr, o[2].ptr, n, br, 7.5, 1.5, *COEFFS, 0.8, S()), "ae_ddim_step_f32")
            return tuple(b.done("ddim_step") for b in o)
        r = ops.ddim_step(xd, ed, COEFFS, br, s0=7.5, s1=1.5, noise=nd, temperature=0.8, want_e=bool(c["want_e"]))
        return tuple(t.cpu() for t in r)
    got = twice(run, "ddim_step")
    assert len(got) == (3 if c["want_e"] or c.get("wrap") else 2)
    for gt, rf, nm in zip(got, ref, ("x_prev", "pred_x0", "e")):
        bits("ae_ddim_step_f32", gt, rf, nm)
    if not c.get("wrap"):
        st = SI.ddim_step(x, eps, COEFFS, br, 7.5, 1.5, nz, 0.8)
        bits("ae_ddim_step_f32", got[0], st[0].contiguous(), "against the stand-in")
        if not c["noise"] and not c["want_e"]:
            x_only = ops.ddim_step(xd, ed, COEFFS, br, s0=7.5, s1=1.5, temperature=0.8, want_pred_x0=False)
            assert x_only[1] is None
            bits("ae_ddim_step_f32", x_only[0].cpu(), ref[0], "without pred_x0")


@cases("ae_ddim_encode_step_f32")
def test_ddim_encode_step(ops, c):
    g = R.gen(110)
    n, br = c["n"], c["branches"]
    shape = (n,) if c.get("wrap") else (3, 4, 5, 7)
    x, eps = R.randn(g, *shape), R.randn(g, br * shape[0], *shape[1:])
    cx, ce = R.c32(1.0123), R.c32(-0.0456)
    xd, ed = d(x), d(eps)

    def run():
        if c.get("wrap"):
            o = Buf(shape, F32)
            ops.check(ops.lib.ae_ddim_encode_step_f32(P(xd), P(ed), o.ptr, n, br, 7.5, cx, ce, S()), "ae_ddim_encode_step_f32")
            return o.done("encode")
        return ops.ddim_encode_step(xd, ed, cx, ce, br, 7.5).cpu()
    got = twice(run, "ddim_encode_step")
    bits("ae_ddim_encode_step_f32", got, R.ref_ddim_encode_step(x, eps, cx, ce, br, 7.5))
    bits("ae_ddim_encode_step_f32", got, SI.ddim_encode_step(x, eps, cx, ce, br, 7.5).contiguous(), "against the stand-in")


@cases("ae_plms_combine_f32")
def test_plms_combine(ops, c):
    g = R.gen(120)
    n, hist = c["n"], c["hist"]
    shape = (n,) if c.get("wrap") else (3, 4, 5, 7)
    e = R.randn(g, *shape)
    olds = [R.randn(g, *shape) for _ in range(max(hist, 1))]
    ed, od = d(e), [d(o) for o in olds]

    def run():
        if c.get("wrap"):
            o = Buf(shape, F32)
            ops.check(ops.lib.ae_plms_combine_f32(P(ed), P(od[3]), P(od[2]), P(od[1]), o.ptr, n, 3, S()), "ae_plms_combine_f32")
            return o.done("plms")
        return (ops.plms_combine_first(ed, od[0]) if hist == 0 else ops.plms_combine(ed, od)).cpu()
    got = twice(run, "plms_combine")
    if hist == 0:
        bits("ae_plms_combine_f32", got, R.ref_plms(e, olds, 0), "first")
        bits("ae_plms_combine_f32", got, SI.plms_combine_first(e, olds[0]), "against the stand-in")
    else:
        bits("ae_plms_combine_f32", got, R.ref_plms_combine(e, olds), f"history {hist}")
        bits("ae_plms_combine_f32", got, SI.plms_combine(e, olds), "against the stand-in")
    if hist == 4:
        bits("ae_plms_combine_f32", got, R.ref_plms(e, [olds[3], olds[2], olds[1]], 3), "the newest three of four")


@cases("ae_mask_blend_f32")
def test_mask_blend(ops, c):
    g = R.gen(130)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    img, x0, nz = (R.randn(g, B, C, H, W) for _ in range(3))
    mshape = {"B1": (B, 1, H, W), "11": (1, 1, H, W), "BC": (B, C, H, W)}[c["mask"]]
    m = torch.rand(*mshape, generator=g)
    m[..., 0] = (m[..., 0] > 0.5).float()                      # hard 0 / 1 values beside soft ones
    sa, s1 = R.c32(0.73), R.c32(0.68)
    a = [d(t) for t in (img, x0, nz, m)]

    def run():
        if c.get("wrap"):
            o = Buf((B, C, H, W), F32)
            ops.check(ops.lib.ae_mask_blend_f32(P(a[0]), P(a[1]), P(a[2]), P(a[3]), o.ptr, B, C, H * W, sa, s1, c["order"], S()), "ae_mask_blend_f32")
            return o.done("mask_blend")
        return ops.mask_blend(*a, sa, s1, ip2p_order=bool(c["order"])).cpu()
    got = twice(run, "mask_blend")
    bits("ae_mask_blend_f32", got, R.ref_mask_blend(img, x0, nz, m, sa, s1, bool(c["order"])))
    bits("ae_mask_blend_f32", got, SI.mask_blend(img, x0, nz, m, sa, s1, bool(c["order"])), "against the stand-in")


@cases("ae_q_sample_f32")
def test_q_sample(ops, c):
    g = R.gen(140)
    B, per = c["B"], c["per"]
    x0, nz = R.randn(g, B, per), R.randn(g, B, per)
    sa, s1 = torch.tensor([0.73, 0.2, 0.99]), torch.tensor([0.68, 0.97, 0.1])
    a = [d(t) for t in (x0, nz, sa, s1)]

    def run():
        if c.get("wrap"):
            o = Buf((B, per), F32)
            ops.check(ops.lib.ae_q_sample_f32(P(a[0]), P(a[1]), P(a[2]), P(a[3]), o.ptr, B, per, S()), "ae_q_sample_f32")
            return o.done("q_sample")
        return ops.q_sample(*a).cpu()
    got = twice(run, "q_sample")
    bits("ae_q_sample_f32", got, R.ref_q_sample(x0, nz, sa, s1))
    bits("ae_q_sample_f32", got, SI.q_sample(x0, nz, sa, s1), "against the stand-in")


@cases("ae_dpm_multistep_f32")
def test_dpm_multistep(ops, c):
    g = R.gen(150)
    n, br = c["n"], c["branches"]
    shape = (n,) if c.get("wrap") else (3, 4, 5, 7)
    x, out, mp = R.randn(g, *shape), R.randn(g, br * shape[0], *shape[1:]), R.randn(g, *shape)
    upd = {"none": None, "first": (1.07, 0.31, 0.0, 0.0), "second": (1.07, 0.31, 0.155, 1.9)}[c["update"]]
    upd = None if upd is None else tuple(R.c32(v) for v in upd)
    sc, sg, al = R.c32(7.5), R.c32(0.61), R.c32(0.79)
    kw = dict(predict_x0=bool(c["predict_x0"]), v_param=bool(c["v_param"]), m_prev=mp if c["update"] == "second" else None, update=upd)
    xd, od, md = d(x), d(out), d(kw["m_prev"])
    if upd is None and not c["want_m"]:
        rejects(ops, lambda: ops.dpm_multistep(xd, od, br, sc, sg, al, want_m=False))     # nothing to write: refused before the launch
        return

    def run():
        if c.get("wrap"):
            m, xn = Buf(shape, F32), Buf(shape, F32)
            ops.check(ops.lib.ae_dpm_multistep_f32(P(xd), P(od), P(md), m.ptr, xn.ptr, n, br, sc, c["v_param"], c["predict_x0"], sg, al, 1, *upd, S()),
                      "ae_dpm_multistep_f32")
            return m.done("m"), xn.done("x_next")
        m, xn = ops.dpm_multistep(xd, od, br, sc, sg, al, predict_x0=kw["predict_x0"], v_param=kw["v_param"], m_prev=md, update=upd, want_m=bool(c["want_m"]))
        return (None if m is None else m.cpu()), (None if xn is None else xn.cpu())
    m, xn = twice(run, "dpm_multistep")
    rm, rx = R.ref_dpm_multistep(x, out, br, sc, sg, al, **kw)
    sm, sx = SI.dpm_multistep(x, out, br, sc, sg, al, **kw)
    assert (m is None) == (not c["want_m"]) and (xn is None) == (upd is None)
    if m is not None:
        bits("ae_dpm_multistep_f32", m, rm, "m")
        bits("ae_dpm_multistep_f32", m, sm.contiguous(), "m against the stand-in")
    if xn is not None:
        bits("ae_dpm_multistep_f32", xn, rx, "x_next")
        bits("ae_dpm_multistep_f32", xn, sx.contiguous(), "x_next against the stand-in")


@cases("ae_lincomb4_f32")
def test_lincomb(ops, c):
    g = R.gen(160 + c["n"] % 13)
    n, k = c["n"], c["terms"]
    ts = [(R.randn(g, n), cf) for cf in (1.3, -0.4, 0.07, 2.5)[:k]]
    td = [(d(t), cf) for t, cf in ts]
    ref, bnd = R.ref_lincomb(ts)

    def run():
        o = Buf((n,), F32)
        assert ops.lincomb(td, out=o.t) is o.t
        return o.done("lincomb")
    near("ae_lincomb4_f32", twice(run, "lincomb"), ref, bnd)
    near("ae_lincomb4_f32", ops.lincomb(td).cpu(), ref, bnd, "fresh output")
    alias = td[0][0].clone()                                     # out= aliasing term 0: every element is read before it is written
    ops.lincomb([(alias, td[0][1])] + td[1:], out=alias)
    near("ae_lincomb4_f32", alias.cpu(), ref, bnd, "out aliases term 0")


def test_lincomb_rejects_a_misaligned_view_before_any_launch(ops):
    t = torch.zeros(1032, device=DEV)
    ok = t[4:1028]
    ops.lincomb([(ok, 1.0)])
    for bad in ([(t[1:1025], 1.0)], [(ok, 1.0), (t[1:1025], 2.0)]):
        rejects(ops, lambda: ops.lincomb(bad))
    rejects(ops, lambda: ops.lincomb([(ok, 1.0)], out=t[1:1025]))
    rejects(ops, lambda: ops.lincomb([]))
    rejects(ops, lambda: ops.lincomb([(ok, 1.0)] * 5))


@cases("ae_dpm_adaptive_err_f32")
def test_dpm_adaptive_err(ops, c):
    xl, xh, xp, atol, rtol = R.adaptive_case(c)
    ref, bnd = R.ref_dpm_adaptive_err(xl, xh, xp, atol, rtol)
    a = [d(t) for t in (xl, xh, xp)]

    def run():
        o = Buf((c["B"],), F32)
        ops.check(ops.lib.ae_dpm_adaptive_err_f32(P(a[0]), P(a[1]), P(a[2]), atol, rtol, c["B"], c["n"], o.ptr, S()), "ae_dpm_adaptive_err_f32")
        return o.done("adaptive_err")
    near("ae_dpm_adaptive_err_f32", twice(run, "dpm_adaptive_err"), ref, bnd)
    near("ae_dpm_adaptive_err_f32", ops.dpm_adaptive_err(*a, atol, rtol).cpu(), ref, bnd, "wrapper")


# ====================================================================================================== layout
@cases("ae_transpose_last2")
def test_transpose(ops, c):
    g = R.gen(200)
    B, X, Y, Xpad = 2, c["X"], c["Y"], c["Xpad"]
    din, dout = (BF if c["in_bf16"] else F32), (BF if c["out_bf16"] else F32)
    x = R.randn(g, B, X, Y, dtype=din)
    xd = d(x)

    def run():
        o = Buf((B, Y, Xpad), dout)
        ops.check(ops.lib.ae_transpose_last2(P(xd), o.ptr, B, X, Y, Xpad, c["in_bf16"], c["out_bf16"], S()), "ae_transpose_last2")
        return o.done("transpose")
    got = twice(run, "transpose")
    ref = R.ref_transpose(x, Xpad, dout)
    bits("ae_transpose_last2", got, ref)
    assert bool((got[:, :, X:].view(torch.int16 if dout == BF else torch.int32) == 0).all()), "padding is not +0"
    # the three wrappers on the same operand: [B, C = X, H = 1, W = Y] -> rows [B Y, Xpad]; rows [B X, Y] -> [B, Y, 1, X]
    if c["out_bf16"]:
        bits("ae_transpose_last2", ops.nchw_to_rows(xd.reshape(B, X, 1, Y), c_pad=Xpad).cpu(), ref.reshape(B * Y, Xpad), "nchw_to_rows")
    nchw = R.ref_transpose(x, X, dout).reshape(B, Y, 1, X)
    bits("ae_transpose_last2", ops.rows_to_nchw(xd.reshape(B * X, Y), B, 1, X, out_dtype=dout).cpu(), nchw, "rows_to_nchw")
    if c["in_bf16"]:
        o = Buf((B, Y, 1, X), dout)
        assert ops.rows_to_nchw_out(xd.reshape(B * X, Y), o.t) is o.t
        bits("ae_transpose_last2", o.done("rows_to_nchw_out"), nchw, "rows_to_nchw_out")


@cases("ae_concat_channels_bf16")
def test_concat_channels(ops, c):
    g = R.gen(210)
    Ca, Cb, rows = c["Ca"], c["Cb"], c["rows"]
    a, b = R.randn(g, rows, Ca, dtype=BF), R.randn(g, rows, Cb, dtype=BF)
    ad, bd = d(a), d(b)

    def run():
        o = Buf((rows, Ca + Cb))
        ops.check(ops.lib.ae_concat_channels_bf16(P(ad), Ca, P(bd), Cb, o.ptr, rows, S()), "ae_concat_channels_bf16")
        return o.done("concat")
    ref = torch.cat([a, b], 1)
    bits("ae_concat_channels_bf16", twice(run, "concat"), ref)
    if not c.get("wrap"):
        bits("ae_concat_channels_bf16", ops.concat_channels(ad, bd).cpu(), ref, "wrapper")


@cases("ae_split_channels_bf16")
def test_split_channels(ops, c):
    g = R.gen(220)
    Ca, Cb, rows, acc, want = c["Ca"], c["Cb"], c["rows"], c["acc"], c["want"]
    dy, oa, ob = R.randn(g, rows, Ca + Cb, dtype=BF), R.randn(g, rows, Ca, dtype=BF), R.randn(g, rows, Cb, dtype=BF)
    dyd = d(dy)
    (ra, ba), (rb, bb) = R.ref_split(dy, Ca, oa if acc else None, ob if acc else None)

    def run():
        ta = Buf((rows, Ca), fill=d(oa) if acc else None) if "a" in want else None
        tb = Buf((rows, Cb), fill=d(ob) if acc else None) if "b" in want else None
        if acc:                                                                       # the wrapper accumulates into the buffers it is given
            ga, gb = ops.split_channels(dyd, Ca, a=ta.t if ta else None, b=tb.t if tb else None, want_a=ta is not None, want_b=tb is not None)
            assert (ga is None) == (ta is None) and (gb is None) == (tb is None)
        else:
            ops.check(ops.lib.ae_split_channels_bf16(P(dyd), Ca, Cb, ta.ptr if ta else None, tb.ptr if tb else None, rows, 0, 0, S()), "ae_split_channels_bf16")
        return (ta.done("da") if ta else None), (tb.done("db") if tb else None)
    ga, gb = twice(run, "split_channels")
    for got, ref, bnd, nm in ((ga, ra, ba, "da"), (gb, rb, bb, "db")):
        if got is None:
            continue
        if acc:
            near("ae_split_channels_bf16", got, ref, bnd, nm)
        else:
            bits("ae_split_channels_bf16", got, ref, nm)
    if not acc and not c.get("wrap"):
        wa, wb = ops.split_channels(dyd, Ca, want_a="a" in want, want_b="b" in want)
        for got, ref, on in ((wa, ra, "a" in want), (wb, rb, "b" in want)):
            assert (got is not None) == on
            if on:
                bits("ae_split_channels_bf16", got.cpu(), ref, "wrapper")


@cases("ae_im2col3x3_c8_bf16")
def test_im2col3x3_c8(ops, c):
    g = R.gen(230)
    B, H, W = c["B"], c["H"], c["W"]
    rows = R.randn(g, B * H * W, 8, dtype=BF)
    rd = d(rows)

    def run():
        o = Buf((B * H * W, 128))
        ops.check(ops.lib.ae_im2col3x3_c8_bf16(P(rd), o.ptr, B, H, W, S()), "ae_im2col3x3_c8_bf16")
        return o.done("im2col")
    ref = R.ref_im2col3x3_c8(rows, B, H, W)
    bits("ae_im2col3x3_c8_bf16", twice(run, "im2col"), ref)
    if not c.get("wrap"):
        bits("ae_im2col3x3_c8_bf16", ops.im2col3x3_c8(rd, B, H, W).cpu(), ref, "wrapper")


@cases("ae_patchify_f32_bf16")
def test_patchify(ops, c):
    g = R.gen(240)
    B, Cin, H, W, Pp = c["B"], c["Cin"], c["H"], c["W"], c["P"]
    x = R.randn(g, B, Cin, H, W)
    xd = d(x)

    def run():
        o = Buf((B * (H // Pp) * (W // Pp), Cin * Pp * Pp))
        ops.check(ops.lib.ae_patchify_f32_bf16(P(xd), o.ptr, B, Cin, H, W, Pp, S()), "ae_patchify_f32_bf16")
        return o.done("patchify")
    ref = R.ref_patchify(x, Pp)
    bits("ae_patchify_f32_bf16", twice(run, "patchify"), ref)
    if not c.get("wrap"):
        bits("ae_patchify_f32_bf16", ops.patchify(xd, Pp).cpu(), ref, "wrapper")
        conv = torch.nn.functional.unfold(x.to(BF).float(), Pp, stride=Pp).transpose(1, 2).reshape(ref.shape)     # (c, ky, kx) = the conv weight's order
        bits("ae_patchify_f32_bf16", ref.float(), conv, "the reference against unfold")


@cases("ae_window_partition_bf16")
def test_window_partition_and_reverse(ops, c):
    g = R.gen(250)
    B, H, W, ws, C = c.get("B", 2), c["H"], c["W"], c["ws"], c["C"]
    x = R.randn(g, B * H * W, C, dtype=BF)
    idx = R.window_index(B, H, W, ws)
    win_in = R.randn(g, idx.numel(), C, dtype=BF)             # the reverse reads windows whose padding rows hold values it must drop
    xd, wd = d(x), d(win_in)

    def run():
        o, r = Buf((idx.numel(), C)), Buf((B * H * W, C))
        ops.check(ops.lib.ae_window_partition_bf16(P(xd), o.ptr, B, H, W, C, ws, 0, S()), "ae_window_partition_bf16")
        ops.check(ops.lib.ae_window_partition_bf16(r.ptr, P(wd), B, H, W, C, ws, 1, S()), "ae_window_partition_bf16")
        return o.done("partition"), r.done("unpartition")
    win, back = twice(run, "window")
    bits("ae_window_partition_bf16", win, R.ref_window_partition(x, B, H, W, ws), "partition")
    assert bool((win[idx < 0].view(torch.int16) == 0).all()), "padding rows are not +0"
    bits("ae_window_partition_bf16", back, R.ref_window_unpartition(win_in, B, H, W, ws), "reverse")
    if not c.get("wrap"):
        w2, (Hp, Wp) = ops.window_partition(xd, B, H, W, ws)
        assert (Hp, Wp) == (-(-H // ws) * ws, -(-W // ws) * ws)
        bits("ae_window_partition_bf16", w2.cpu(), win, "wrapper")
        bits("ae_window_partition_bf16", ops.window_unpartition(w2, B, H, W, ws).cpu(), x, "round trip")


# ====================================================================================================== UNet glue
@cases("ae_silu_to_bf16")
def test_silu_to_bf16(ops, c):
    g = R.gen(300)
    n = c["n"]
    x = (torch.rand(n, generator=g) * 200 - 100)
    x[:5] = torch.tensor([0.0, -0.0, 100.0, -100.0, 1e-3])
    x = x.to(BF) if c["in_bf16"] else x
    xd = d(x)

    def run():
        o = Buf((n,))
        ops.check(ops.lib.ae_silu_to_bf16(P(xd), c["in_bf16"], o.ptr, n, S()), "ae_silu_to_bf16")
        return o.done("silu")
    ref, bnd = R.ref_silu(x)
    near("ae_silu_to_bf16", twice(run, "silu"), ref, bnd)
    if not c.get("wrap"):
        near("ae_silu_to_bf16", ops.silu_to_bf16(xd).cpu(), ref, bnd, "wrapper")


@cases("ae_add_bcast_bf16")
def test_add_bcast(ops, c):
    g = R.gen(310)
    period, reps = c["period"], c["reps"]
    x, p = R.randn(g, reps, period, dtype=BF), R.randn(g, period, dtype=BF)
    xd, pd = d(x), d(p)

    def run():
        o = Buf((reps, period))
        ops.check(ops.lib.ae_add_bcast_bf16(P(xd), P(pd), o.ptr, reps * period, period, S()), "ae_add_bcast_bf16")
        return o.done("add_bcast")
    ref, bnd = R.ref_add_bcast(x, p)
    near("ae_add_bcast_bf16", twice(run, "add_bcast"), ref, bnd)
    if not c.get("wrap"):
        near("ae_add_bcast_bf16", ops.add_bcast(xd, pd).cpu(), ref, bnd, "wrapper")


@cases("ae_resample2x_rows_bf16")
def test_resample2x_rows(ops, c):
    g = R.gen(320)
    B, H, W, C, down = c["B"], c["H"], c["W"], c["C"], c["down"]
    x = R.randn(g, B * H * W, C, dtype=BF)
    xd = d(x)
    Ho, Wo = (H // 2, W // 2) if down else (2 * H, 2 * W)

    def run():
        o = Buf((B * Ho * Wo, C))
        ops.check(ops.lib.ae_resample2x_rows_bf16(P(xd), o.ptr, B, H, W, C, down, S()), "ae_resample2x_rows_bf16")
        return o.done("resample")
    got = twice(run, "resample2x_rows")
    if down:
        ref, bnd = R.ref_mean2x2(x, B, H, W)
        near("ae_resample2x_rows_bf16", got, ref, bnd, "2x2 mean")
    else:
        bits("ae_resample2x_rows_bf16", got, R.ref_nearest2x(x, B, H, W), "nearest")
    if not c.get("wrap"):
        w, ho, wo = ops.resample2x_rows(xd, B, H, W, down=bool(down))
        assert (ho, wo) == (Ho, Wo)
        bits("ae_resample2x_rows_bf16", w.cpu(), got, "wrapper")


@cases("ae_scale_shift_rows_bf16")
def test_scale_shift_rows(ops, c):
    g = R.gen(330)
    B, HW, C, silu = c["B"], c["HW"], c["C"], c["silu"]
    x = R.randn(g, B * HW, C, dtype=BF)
    wide = R.randn(g, B, 2 * C + 24)                          # emb: a column slice of a wider projection, ld > 2C
    emb = wide[:, 8:8 + 2 * C]
    xd, ed = d(x), d(wide)[:, 8:8 + 2 * C]
    assert ed.stride(0) > 2 * C

    def run():
        o = Buf((B * HW, C))
        ops.check(ops.lib.ae_scale_shift_rows_bf16(P(xd), P(ed), ed.stride(0), o.ptr, B, HW, C, silu, S()), "ae_scale_shift_rows_bf16")
        return o.done("scale_shift")
    ref, bnd = R.ref_scale_shift(x, emb, B, HW, bool(silu))
    near("ae_scale_shift_rows_bf16", twice(run, "scale_shift_rows"), ref, bnd)
    if not c.get("wrap"):
        near("ae_scale_shift_rows_bf16", ops.scale_shift_rows(xd, ed, B, HW, silu=bool(silu)).cpu(), ref, bnd, "wrapper")


@cases("ae_softmax_rows_f32_bf16")
def test_softmax_rows(ops, c):
    g = R.gen(340 + c["cols"] % 11)
    rows, cols, scale = 3, c["cols"], c["scale"]
    wide = (torch.rand(rows, cols + 5, generator=g) * 160 - 80)
    wide[0, :cols] = wide[0, 0]                                 # a constant row: every probability 1 / cols
    Sv = wide[:, :cols]
    Sd = d(wide)[:, :cols]
    assert cols == 1 or Sd.stride(0) > cols

    def run():
        o = Buf((rows, cols), ld=cols + 3)
        ops.check(ops.lib.ae_softmax_rows_f32_bf16(P(Sd), Sd.stride(0), o.ptr, cols + 3, rows, cols, scale, S()), "ae_softmax_rows_f32_bf16")
        return o.done("softmax")
    ref, bnd = R.ref_softmax_rows(Sv, scale)
    near("ae_softmax_rows_f32_bf16", twice(run, "softmax_rows"), ref, bnd)
    near("ae_softmax_rows_f32_bf16", ops.softmax_rows(Sd, scale).cpu(), ref, bnd, "wrapper")


@cases("ae_gaussian_moments_f32")
def test_gaussian_moments(ops, c):
    g = R.gen(350)
    B, per = c["B"], c["per"]
    Cz = 5 if per == 35 else 1
    hw = per // Cz
    lv = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0])[torch.randint(0, 5, (B, Cz, hw), generator=g)] + 0.0
    lv[:, :, -1] = R.randn(g, B, Cz)                             # and ordinary values
    mom = torch.cat([R.randn(g, B, Cz, hw), lv], 1)
    nz = R.randn(g, B, Cz, hw) if c["noise"] else None
    md, nd = d(mom), d(nz)
    f = R.ref_gaussian(mom, nz)
    stats = bool(c["want_stats"])

    def run():
        if c.get("wrap"):
            o = [Buf((B, Cz, hw), F32) for _ in range(4)]
            ops.check(ops.lib.ae_gaussian_moments_f32(P(md), P(nd), *(b.ptr for b in o), B, per, S()), "ae_gaussian_moments_f32")
            return tuple(b.done("gaussian") for b in o)
        r = ops.gaussian_moments(md, noise=nd, want_stats=stats)
        return tuple(t.cpu() for t in r) if stats else (r.cpu(),)
    got = twice(run, "gaussian_moments")
    assert len(got) == (4 if stats or c.get("wrap") else 1)
    if nz is None:
        bits("ae_gaussian_moments_f32", got[0], f["mean"].float().contiguous(), "the mode")
    else:
        near("ae_gaussian_moments_f32", got[0], f["z"], R.bound_c32(f["z"]), "z")
    if len(got) == 4:
        bits("ae_gaussian_moments_f32", got[1], f["mean"].float().contiguous(), "mean")
        bits("ae_gaussian_moments_f32", got[2], f["logvar"].float().contiguous(), "logvar clamped at both ends")
        near("ae_gaussian_moments_f32", got[3], f["std"], R.bound_c32(f["std"]), "std")
        assert float(got[2].min()) == -30.0 and float(got[2].max()) == 20.0


@cases("ae_timestep_embedding")
def test_timestep_embedding(ops, c):
    dim, mp = c["dim"], c["max_period"]
    t = torch.tensor([0, 1, 21, 500, 981, 999]) if c["kind"] == "i64" else torch.tensor([0.0, 999.5, 0.25, 500.0, 21.75])
    td = d(t)
    ref = R.ref_timestep_embedding(t, dim, mp)

    def run():
        return ops.timestep_embedding(td, dim, max_period=mp, out_f32=True).cpu(), ops.timestep_embedding(td, dim, max_period=mp).cpu()
    f32, bf = twice(run, "timestep_embedding")
    near("ae_timestep_embedding", f32, ref, R.TIMESTEP_TOL)
    R.check_bits(bf, f32.to(BF), "the bf16 output is the fp32 output rounded")
    if dim % 2:
        assert bool((f32[:, -1].view(torch.int32) == 0).all()), "the odd column is +0"
    o32, o16 = Buf(tuple(ref.shape), F32), Buf(tuple(ref.shape))          # both outputs of one launch
    ti, tf = (td, None) if c["kind"] == "i64" else (None, td)
    ops.check(ops.lib.ae_timestep_embedding(P(ti), P(tf), o16.ptr, o32.ptr, t.numel(), dim, mp, S()), "ae_timestep_embedding")
    R.check_bits(o32.done("fp32"), f32, "both outputs: fp32")
    R.check_bits(o16.done("bf16"), bf, "both outputs: bf16")


@cases("ae_sam_relpos_terms")
def test_sam_relpos_terms(ops, c):
    g = R.gen(c["seed"])
    B, heads, D, qH, qW, kH, kW = 2, 3, c["D"], c["qH"], c["qW"], c["kH"], c["kW"]
    N = qH * qW
    assert (B * heads * qW) % 64 and (B * heads * qH) % 64
    qkv = R.randn(g, B, N, 3, heads, D, dtype=BF)                # q: a strided view of the fused qkv rows
    Rh, Rw = R.randn(g, qH, kH, D), R.randn(g, qW, kW, D)
    strides = (N * 3 * heads * D, D, 3 * heads * D)
    mfma = D % 16 == 0 and D <= 96 and all(s % 4 == 0 for s in strides)
    line = qH <= 64 and qW <= 64 and kH <= 64 and kW <= 64 and D % 8 == 0 and D <= 160 and all(s % 8 == 0 for s in strides)
    assert ("mfma" if mfma else "line" if line else "generic") == c["route"], "the shape does not select the route the case is for"
    qd, hd, wd = d(qkv), d(Rh), d(Rw)

    def run():
        oh, ow = Buf((B * heads, N, kH), F32), Buf((B * heads, N, kW), F32)
        ops.check(ops.lib.ae_sam_relpos_terms(P(qd), *strides, P(hd), P(wd), oh.ptr, ow.ptr, B, heads, qH, qW, kH, kW, D, S()), "ae_sam_relpos_terms")
        return oh.done("rel_h"), ow.done("rel_w")
    gh, gw = twice(run, "sam_relpos_terms")
    (rh, bh), (rw, bw) = R.ref_relpos(qkv[:, :, 0], Rh, Rw, qH, qW)
    near("ae_sam_relpos_terms", gh, rh, bh, f"rel_h ({c['route']})")
    near("ae_sam_relpos_terms", gw, rw, bw, f"rel_w ({c['route']})")
    wh, ww = ops.sam_relpos_terms(qd, strides, hd, wd, B, heads, qH, qW, D)
    R.check_bits(wh.cpu(), gh, "wrapper rel_h")
    R.check_bits(ww.cpu(), gw, "wrapper rel_w")


# ====================================================================================================== backward.hip
@cases("ae_add_bf16")
def test_add(ops, c):
    g = R.gen(400)
    n = c["n"]
    a, b = R.randn(g, n, dtype=BF), R.randn(g, n, dtype=BF)
    ad, bd = d(a), d(b)

    def run():
        o = Buf((n,))
        assert ops.add(ad, bd, out=o.t) is o.t
        return o.done("add")
    ref, bnd = R.ref_axpy(a, b, 1.0)
    near("ae_add_bf16", twice(run, "add"), ref, bnd)
    if not c.get("wrap"):
        near("ae_add_bf16", ops.add(ad, bd).cpu(), ref, bnd, "fresh output")


@cases("ae_axpy_bf16")
def test_axpy(ops, c):
    g = R.gen(410)
    n, alpha = c["n"], c["alpha"]
    a, b = R.randn(g, n, dtype=BF), R.randn(g, n, dtype=BF)
    ad, bd = d(a), d(b)

    def run():
        o = Buf((n,))
        assert ops.axpy(ad, bd, alpha, out=o.t) is o.t
        return o.done("axpy")
    ref, bnd = R.ref_axpy(a, b, alpha)
    near("ae_axpy_bf16", twice(run, "axpy"), ref, bnd)


def test_add_axpy_reject_a_length_off_the_vector_width_before_any_launch(ops):
    a = torch.zeros(2056 + 4, dtype=BF, device=DEV)
    for n in (4, 2052, 2060):
        rejects(ops, lambda: ops.add(a[:n], a[:n]))
        rejects(ops, lambda: ops.axpy(a[:n], a[:n], 0.5))


@cases("ae_geglu_fwd_bf16")
def test_geglu(ops, c):
    g = R.gen(420)
    M, F = c["M"], c["F"]
    h = torch.cat([R.randn(g, M, F), torch.rand(M, F, generator=g) * 12 - 6], 1).to(BF)      # gate values in +-6
    hd = d(h)

    def run():
        o = Buf((M, F))
        ops.check(ops.lib.ae_geglu_fwd_bf16(P(hd), o.ptr, M, F, S()), "ae_geglu_fwd_bf16")
        return o.done("geglu")
    ref, bnd = R.ref_geglu(h)
    near("ae_geglu_fwd_bf16", twice(run, "geglu"), ref, bnd)
    if not c.get("wrap"):
        near("ae_geglu_fwd_bf16", ops.geglu(hd).cpu(), ref, bnd, "wrapper")


@cases("ae_geglu_bwd_bf16")
def test_geglu_bwd(ops, c):
    g = R.gen(430)
    M, F = c["M"], c["F"]
    h = torch.cat([R.randn(g, M, F), torch.rand(M, F, generator=g) * 12 - 6], 1).to(BF)
    dy = R.randn(g, M, F, dtype=BF)
    hd, dyd = d(h), d(dy)

    def run():
        o = Buf((M, 2 * F))
        ops.check(ops.lib.ae_geglu_bwd_bf16(P(hd), P(dyd), o.ptr, M, F, S()), "ae_geglu_bwd_bf16")
        return o.done("geglu_bwd")
    ref, bnd = R.ref_geglu_bwd(h, dy)
    near("ae_geglu_bwd_bf16", twice(run, "geglu_bwd"), ref, bnd)
    if not c.get("wrap"):
        near("ae_geglu_bwd_bf16", ops.geglu_bwd(hd, dyd).cpu(), ref, bnd, "wrapper")
        if M * F <= 4096:                                      # float64 autograd of the forward, as the reference is checked on the CPU
            hh = h.to(F64).requires_grad_(True)
            (hh[:, :F] * torch.nn.functional.gelu(hh[:, F:])).backward(dy.to(F64))
            assert float((ref - hh.grad).abs().max()) <= 1e-12


@cases("ae_sumpool2x2_bf16")
def test_sumpool2x2(ops, c):
    g = R.gen(440)
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    x = R.randn(g, B * 2 * H * 2 * W, C, dtype=BF)
    xd = d(x)

    def run():
        o = Buf((B * H * W, C))
        ops.check(ops.lib.ae_sumpool2x2_bf16(P(xd), o.ptr, B, H, W, C, S()), "ae_sumpool2x2_bf16")
        return o.done("sumpool")
    ref, bnd = R.ref_sumpool2x2(x, B, H, W)
    near("ae_sumpool2x2_bf16", twice(run, "sumpool2x2"), ref, bnd)
    if not c.get("wrap"):
        near("ae_sumpool2x2_bf16", ops.sumpool2x2(xd, B, H, W).cpu(), ref, bnd, "wrapper")


@cases("ae_colsum_bf16_f32")
def test_colsum(ops, c):
    g = R.gen(450)
    M, N, ld = c["M"], c["N"], c["ld"]
    wide = R.randn(g, M, ld, dtype=BF)
    x = wide[:, :N]
    xd = d(wide)[:, :N]

    def run():
        o = Buf((N,), F32)
        ops.check(ops.lib.ae_colsum_bf16_f32(P(xd), o.ptr, M, N, ld, S()), "ae_colsum_bf16_f32")
        return o.done("colsum")
    ref, bnd = R.ref_colsum(x)
    near("ae_colsum_bf16_f32", twice(run, "colsum"), ref, bnd)
    near("ae_colsum_bf16_f32", ops.colsum(xd).cpu(), ref, bnd, "wrapper")


@cases("ae_mse_f32")
def test_mse(ops, c):
    g = R.gen(460)
    n = c["n"]
    a, b = R.randn(g, n), R.randn(g, n) * 0.5
    ad, bd = d(a), d(b)

    def run():
        o, part = Buf((1,), F32), Buf((1024,), F32, fill=torch.zeros(1024, device=DEV))      # scratch: only its guards are checked
        ops.check(ops.lib.ae_mse_f32(P(ad), P(bd), o.ptr, part.ptr, n, S()), "ae_mse_f32")
        part.done("mse scratch")
        return o.done("mse")
    ref, bnd = R.ref_mse(a, b)
    near("ae_mse_f32", twice(run, "mse").reshape(()), ref, bnd)
    if not c.get("wrap"):
        near("ae_mse_f32", ops.mse(ad, bd).cpu(), ref, bnd, "wrapper")


@cases("ae_mse_grad_f32")
def test_mse_grad(ops, c):
    g = R.gen(470)
    n, ls = c["n"], c["loss_scale"]
    p, t = R.randn(g, n), R.randn(g, n)
    pd, td = d(p), d(t)

    def run():
        o = Buf((n,), F32)
        ops.check(ops.lib.ae_mse_grad_f32(P(pd), P(td), o.ptr, n, ls, S()), "ae_mse_grad_f32")
        return o.done("mse_grad")
    ref, bnd = R.ref_mse_grad(p, t, ls)
    near("ae_mse_grad_f32", twice(run, "mse_grad"), ref, bnd)
    if not c.get("wrap"):
        near("ae_mse_grad_f32", ops.mse_grad(pd, td, ls).cpu(), ref, bnd, "wrapper")


@cases("ae_adamw_f32")
def test_adamw_step(ops, c):
    g = R.gen(480)
    n, start, wd, gs = c["n"], c["start"], c["weight_decay"], c["grad_scale"]
    lr = 1e-3
    steps = (1, 2, 3) if start == 1 else (1000,)
    p0 = R.randn(g, n)
    m0 = torch.zeros(n) if start == 1 else R.randn(g, n, scale=0.1)
    v0 = torch.zeros(n) if start == 1 else R.randn(g, n).abs() * 0.01
    grads = [R.randn(g, n) / gs for _ in steps]                  # scaled gradients, as a loss scale leaves them
    gd = [d(t) for t in grads]

    def run():
        p, m, v = Buf((n,), F32, fill=d(p0)), Buf((n,), F32, fill=d(m0)), Buf((n,), F32, fill=d(v0))
        hist = []
        for st, gr in zip(steps, gd):
            ops.adamw_step(p.t, gr, m.t, v.t, st, lr, weight_decay=wd, grad_scale=gs)
            hist.append(p.t.cpu().clone())
        return tuple(hist) + (m.done("m"), v.done("v"), p.done("p"))
    got = twice(run, "adamw_step")
    p, m, v = p0, m0, v0                                         # float64 over the same steps, from the same start
    for i, (st, gr) in enumerate(zip(steps, grads)):
        p, m, v = R.ref_adamw(p, gr, m, v, st, lr, weight_decay=wd, grad_scale=gs)
        near("ae_adamw_f32", got[i], p, R.bound_f(p, lr, i + 1), f"p after step {st}")
    gmax = float(max(t.abs().max() for t in grads)) * gs
    R.check_elements(got[-3], m, R.A * (m.abs() + 0.1 * gmax), "exp_avg")
    R.check_elements(got[-2], v, R.A * (v.abs() + 1e-3 * gmax * gmax), "exp_avg_sq")
    if start == 1 and gs == 1.0 and not c.get("wrap"):           # and torch's own optimiser, as tests/test_hip_backward.py does
        pt = p0.clone().requires_grad_(True)
        opt = torch.optim.AdamW([pt], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        for gr in grads:
            pt.grad = gr.clone()
            opt.step()
        assert float((got[len(steps) - 1] - pt.detach()).abs().max()) <= 1e-5


@cases("ae_scatter_add_rows_f32")
def test_scatter_add_rows(ops, c):
    g = R.gen(490)
    D, B, n_rows = c["D"], 6, 7
    src, dst = R.randn(g, B, D), R.randn(g, n_rows, D)
    code = torch.tensor([2, 0, 2, 5, 2, 0], dtype=torch.int32 if c["code_dtype"] == "i32" else torch.int64)
    sd, cd = d(src), d(code)

    def run():
        o = Buf((n_rows, D), F32, fill=d(dst))
        assert ops.scatter_add_rows(sd, cd, o.t) is o.t
        return o.done("scatter")
    got = twice(run, "scatter_add_rows")
    ref, bnd = R.ref_scatter_add_rows(src, code, dst)
    near("ae_scatter_add_rows_f32", got, ref, bnd)
    R.check_bits(got[[1, 3, 4, 6]], dst[[1, 3, 4, 6]], "rows no code names are untouched")


@cases("ae_rowsum_f32")
def test_rowsum_f32(ops, c):
    g = R.gen(500)
    rows, n = c["rows"], c["n"]
    x = R.randn(g, rows, n)
    xd = d(x)

    def run():
        o = Buf((rows,), F32)
        ops.check(ops.lib.ae_rowsum_f32(P(xd), o.ptr, rows, n, S()), "ae_rowsum_f32")
        return o.done("rowsum")
    ref, bnd = R.ref_rowsum(x)
    near("ae_rowsum_f32", twice(run, "rowsum"), ref, bnd)
    near("ae_rowsum_f32", ops.rowsum_f32(xd).cpu(), ref, bnd, "wrapper")


# ====================================================================================================== gate.hip
@cases("ae_task_gate")
def test_task_gate(ops, c):
    te, code, Wg, bg = R.gate_case(c)
    f = R.ref_task_gate(te, code, Wg, bg)
    a = [d(t) for t in (te, code, Wg, bg)]

    def run():
        return tuple(t.cpu() for t in ops.task_gate(*a))
    probs, top1, top1p = twice(run, "task_gate")
    near("ae_task_gate", probs, f["probs"], f["bnd"], "probs")
    assert top1.dtype == torch.int32
    R.check_bits(top1.long(), f["top1"], "top1 (lowest index on ties)")
    near("ae_task_gate", top1p, f["top1_prob"], f["bnd_top1"], "top1_prob")
    R.check_bits(top1p, probs[torch.arange(code.numel()), top1.long()], "top1_prob is the winner's probability")
    assert float((probs.double().sum(-1) - 1).abs().max()) <= 1e-5
    if c.get("tie"):
        assert int(top1[0]) == c["tie"][0] and float(probs[0, c["tie"][0]]) == float(probs[0, c["tie"][1]])


def test_task_gate_rejects_more_experts_than_a_wave_before_any_launch(ops):
    te, code = torch.zeros(6, 48, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    Wg = torch.zeros(65, 48, device=DEV)
    rejects(ops, lambda: ops.task_gate(te, code, Wg, None))
    p = torch.full((4, 65), 1.0 / 65, device=DEV)
    t1, dg = torch.zeros(4, dtype=torch.int32, device=DEV), torch.ones(4, device=DEV)
    rejects(ops, lambda: ops.task_gate_bwd(p, t1, dg, Wg))
    rejects(ops, lambda: ops.task_gate_wgrad(p, t1, dg, te, code))


@cases("ae_task_gate_bwd")
def test_task_gate_bwd_and_wgrad(ops, c):
    te, code, Wg, bg = R.gate_case(c)
    f = R.ref_task_gate(te, code, Wg, bg)
    B = code.numel()
    assert B == 5 and len(set(code.tolist())) < B, "repeated codes"
    p32, top1, dg = f["probs"].float(), f["top1"].to(torch.int32), R.randn(R.gen(5), B)
    a = [d(t) for t in (p32, top1, dg)]

    def run():
        dte = ops.task_gate_bwd(*a, d(Wg))
        dW, db = ops.task_gate_wgrad(*a, d(te), d(code))
        return dte.cpu(), dW.cpu(), db.cpu()
    dte, dW, db = twice(run, "task_gate_bwd / wgrad")
    ref, bnd = R.ref_task_gate_bwd(p32, top1, dg, Wg)
    near("ae_task_gate_bwd", dte, ref, bnd, "dte")
    (rW, bW), (rb, bb) = R.ref_task_gate_wgrad(p32, top1, dg, te, code)
    near("ae_task_gate_wgrad", dW, rW, bW, "dWg")
    near("ae_task_gate_wgrad", db, rb, bb, "dbg")
    # float64 autograd of g_b = softmax(.)[top1_b] with top1 held constant, from the same fp32 probabilities' logits
    rows = te.to(F64)[code.clamp(0, te.shape[0] - 1)].clone().requires_grad_(True)
    W, b = Wg.to(F64).clone().requires_grad_(True), bg.to(F64).clone().requires_grad_(True)
    torch.softmax(rows @ W.t() + b, -1)[torch.arange(B), f["top1"]].backward(dg.to(F64))
    # the kernels read fp32 probabilities: each is off by up to 2^-25, so (1 - p) of a confident winner and every dlogit by up to 2^-23 |dgate|
    dga = dg.to(F64).abs()
    slack = (dga[:, None] * Wg.to(F64).abs().sum(0)[None], (dga[:, None] * rows.detach().abs()).sum(0).expand(Wg.shape[0], -1), dga.sum().expand(Wg.shape[0]))
    for got, auto, bd, sl in zip((dte, dW, db), (rows.grad, W.grad, b.grad), (bnd, bW, bb), slack):
        R.check_elements(got, auto, bd + 2.0 ** -23 * sl, "against autograd (the probabilities rounded to fp32)")


# ====================================================================================================== expert_kv.hip
def expert_operands(c):
    g = R.gen(c["seed"])
    B, T, N, Dc, E = (c[k] for k in ("B", "T", "N", "Dc", "E"))
    x, dy = R.randn(g, B * T, Dc, dtype=BF), R.randn(g, B * T, N, dtype=BF)
    W = R.randn(g, E, N, Dc, scale=Dc ** -0.5)
    return x, dy, W, R.expert_ids(c)


@cases("ae_expert_kv_fwd")
def test_expert_kv(ops, c):
    x, dy, W, ex = expert_operands(c)
    T, E = c["T"], c["E"]
    xd, dyd, Wd, exd = d(x), d(dy), d(W), d(ex)

    def run():
        dW = Buf(tuple(W.shape), F32)
        y, dx = ops.expert_kv(xd, Wd, exd, T), ops.expert_kv_dgrad(dyd, Wd, exd, T)
        assert ops.expert_kv_wgrad(dyd, xd, exd, T, E, out=dW.t) is dW.t
        return y.cpu(), dx.cpu(), dW.done("dW")
    y, dx, dW = twice(run, "expert_kv")
    ref, bnd = R.ref_expert_fwd(x, W, ex, T)
    near("ae_expert_kv_fwd", y, ref, bnd)
    ref, bnd = R.ref_expert_dgrad(dy, W, ex, T)
    near("ae_expert_kv_dgrad", dx, ref, bnd)
    ref, bnd = R.ref_expert_wgrad(dy, x, ex, T, E)
    near("ae_expert_kv_wgrad", dW, ref, bnd)
    used = set(ex.clamp(0, E - 1).tolist())
    for e in range(E):
        if e not in used:
            assert bool((dW[e].view(torch.int32) == 0).all()), f"expert {e} has no sample: dW must be exact +0"
    if c.get("ids") == "one":
        assert used == {E - 1} and E > 1


def test_expert_kv_rejects_unsupported_shapes_before_any_launch(ops):
    def z(*s, dtype=BF):
        return torch.zeros(*s, dtype=dtype, device=DEV)
    ex = torch.zeros(257, dtype=torch.int64, device=DEV)
    rejects(ops, lambda: ops.expert_kv_wgrad(z(257, 16), z(257, 8), ex, 1, 2))                         # B T = 257 rows
    W = z(1, 16, 4100, dtype=F32)
    rejects(ops, lambda: ops.expert_kv(z(2, 4100), W, ex[:2], 1))                                        # Dc = 4100
    rejects(ops, lambda: ops.expert_kv_dgrad(z(2, 16), W, ex[:2], 1))
    rejects(ops, lambda: ops.expert_kv_wgrad(z(2, 16), z(2, 4100), ex[:2], 1, 1))
    rejects(ops, lambda: ops.expert_kv(z(9, 8), z(1, 16, 8, dtype=F32), ex[:1], 9))                      # T = 9 tokens
    rejects(ops, lambda: ops.expert_kv(z(2, 8), z(1, 24, 8, dtype=F32), ex[:2], 1))                      # N off 16


# ====================================================================================================== wrappers: layouts
def _layouts(t):
    """the same values as a dense non-contiguous tensor (channels-last / transposed) and as a 16-byte aligned column slice of a wider buffer"""
    dense = t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.transpose(0, -1).contiguous().transpose(0, -1)
    wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 16, dtype=t.dtype, device=t.device)
    wide[..., 8:8 + t.shape[-1]] = t
    sl = wide[..., 8:8 + t.shape[-1]]
    assert not sl.is_contiguous() and not dense.is_contiguous() and torch.equal(sl, t) and torch.equal(dense, t)
    return dense, sl


def _same_or_refused(fn, args, vary, what):
    """fn(*args) with argument `vary` in another layout: the contiguous result bit for bit, or ValueError / TypeError — never another answer"""
    want = fn(*args)
    want = want if isinstance(want, tuple) else (want,)
    for kind, alt in zip(("dense non-contiguous", "column slice"), _layouts(args[vary])):
        a2 = list(args)
        a2[vary] = alt
        try:
            got = fn(*a2)
        except (ValueError, TypeError):
            continue
        got = got if isinstance(got, tuple) else (got,)
        for u, v in zip(got, want):
            if u is None and v is None:
                continue
            assert u.shape == v.shape, f"{what}: argument {vary} as a {kind}: shape {tuple(u.shape)}"
            assert torch.equal(u.cpu(), v.cpu()), f"{what}: argument {vary} as a {kind} gives a different answer, silently"


LAYOUT_OPS = ("mask_blend", "q_sample", "plms_combine_first", "geglu_bwd", "concat_channels", "split_channels", "add_bcast", "colsum", "softmax_rows",
              "ddim_step", "sam_relpos_terms")


@pytest.mark.parametrize("name", LAYOUT_OPS)
def test_wrappers_take_any_layout_or_refuse_it(ops, name):
    g = R.gen(600)
    img, x0, nz = (d(R.randn(g, 2, 4, 8, 8)) for _ in range(3))
    h, dy = d(R.randn(g, 16, 48, dtype=BF)), d(R.randn(g, 16, 24, dtype=BF))
    a, b = d(R.randn(g, 16, 8, dtype=BF)), d(R.randn(g, 16, 16, dtype=BF))
    if name == "mask_blend":
        mask = d((torch.rand(2, 1, 8, 8, generator=g) > 0.5).float())
        for i in range(3):
            _same_or_refused(lambda u, v, w, m: ops.mask_blend(u, v, w, m, 0.73, 0.68), [img, x0, nz, mask], i, name)
    elif name == "q_sample":
        sa, s1 = d(torch.tensor([0.73, 0.2])), d(torch.tensor([0.68, 0.97]))
        for i in range(2):
            _same_or_refused(lambda u, v: ops.q_sample(u, v, sa, s1), [x0, nz], i, name)
    elif name == "plms_combine_first":
        for i in range(2):
            _same_or_refused(ops.plms_combine_first, [x0, nz], i, name)
    elif name == "geglu_bwd":
        for i in range(2):
            _same_or_refused(ops.geglu_bwd, [h, dy], i, name)
    elif name == "concat_channels":
        for i in range(2):
            _same_or_refused(ops.concat_channels, [a, b], i, name)
        with pytest.raises((ValueError, TypeError)):
            ops.concat_channels(a.float(), b)
    elif name == "split_channels":
        _same_or_refused(lambda t: ops.split_channels(t, 8), [dy], 0, "split_channels.dy")
        want = ops.split_channels(dy, 8, a=a.clone(), b=b.clone())
        for i in range(2):                                       # an accumulation target in another layout: refused, or added to in place
            for alt in _layouts([a, b][i]):
                tg = [a.clone(), b.clone()]
                tg[i] = alt
                try:
                    got = ops.split_channels(dy, 8, a=tg[0], b=tg[1])
                except (ValueError, TypeError):
                    continue
                assert torch.equal(got[i].cpu(), want[i].cpu()), "split_channels: a strided accumulation target gives a different answer"
    elif name == "add_bcast":
        p = d(R.randn(g, 2, 8, dtype=BF))
        for i in range(2):
            _same_or_refused(ops.add_bcast, [a, p], i, name)
        with pytest.raises((ValueError, TypeError)):
            ops.add_bcast(a.float(), p)
    elif name == "colsum":
        _same_or_refused(ops.colsum, [dy], 0, name)
    elif name == "softmax_rows":
        _same_or_refused(lambda t: ops.softmax_rows(t, 0.5), [d(R.randn(g, 8, 24))], 0, name)
    elif name == "ddim_step":
        xs, eps = d(R.randn(g, 2, 4, 8, 8)), d(R.randn(g, 4, 4, 8, 8))
        _same_or_refused(lambda n_: ops.ddim_step(xs, eps, COEFFS, 2, s0=7.5, noise=n_), [nz], 0, "ddim_step.noise")
        with pytest.raises((ValueError, TypeError)):
            ops.ddim_step(xs, eps, COEFFS, 2, s0=7.5, noise=nz.double())
    else:
        qkv = d(R.randn(g, 2, 20, 3, 3, 16, dtype=BF))
        Rh, Rw = d(R.randn(g, 4, 7, 16)), d(R.randn(g, 5, 8, 16))
        st = (20 * 3 * 3 * 16, 16, 3 * 3 * 16)
        for i in range(2):
            _same_or_refused(lambda u, v: ops.sam_relpos_terms(qkv, st, u, v, 2, 3, 4, 5, 16), [Rh, Rw], i, name)
        with pytest.raises((ValueError, TypeError)):
            ops.sam_relpos_terms(qkv, st, Rh.to(BF), Rw, 2, 3, 4, 5, 16)
