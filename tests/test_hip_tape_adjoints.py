"""anyedit_amd/autodiff.py, adjoint by adjoint: a tape of one node (two or three where a fan-out is the point) at the smallest shapes where
the tape's own work can go wrong — transposed weight slices, the rotated and re-padded conv weight, the zero-insert gather and its crop on
odd maps, the 2x2 sums, the zero-padded transposes of dW, the four routes of the concat adjoint, the gradient buffers of the attention node.

  A. adjoints built from forward kernels: every element against the float64 references of tests/tape_ref.py, with the project's bounds
     (composed there where a route stores bf16 more than once);
  B. layout adjoints: bit for bit, or within one rounding where a sum is stored;
  C. adjoints that call a backward kernel (those kernels have route tests of their own): bit for bit against a direct call of the same
     ops.*_bwd wrapper on the same arguments, and the routing around the call is asserted;
  D. refusals: pure Python, raised before any launch.

Inputs are seeded, B = 2 wherever a batch exists.  Every case runs twice and the two results must agree bit for bit.  The module stops at
the first device error.  The worst error / bound per adjoint is printed when the module finishes (`-s`): DESIGN.md's table."""
import collections

import pytest
import torch

import norm_ref as NR
import small_ref as S
import tape_ref as R

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
RATIOS = collections.defaultdict(float)


@pytest.fixture(scope="module")
def ops():
    from anyedit_amd import ops as o
    yield o
    print("\nworst error / bound per adjoint (0 = bit-exact)")
    for k in sorted(RATIOS):
        print(f"  ratio {k:<44s} {RATIOS[k]:.4f}")


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a failed assertion lets the module go on; an error of the device ends it (nothing more is launched on a faulted GPU)"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit(f"GPU error, stopping: {e}", returncode=3)


def Tape():
    from anyedit_amd.autodiff import Tape as T
    return T()


def dv(t, dtype=BF):
    return None if t is None else t.to(dtype).to(DEV)


def cpu(t):
    return None if t is None else t.detach().cpu().contiguous()


def twice(fn, what):
    """fn() -> a CPU tensor, None, or a tuple of them; run twice, bit-equal"""
    a, b = fn(), fn()
    la, lb = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(la) == len(lb)
    for i, (u, v) in enumerate(zip(la, lb)):
        assert (u is None) == (v is None)
        if u is not None:
            S.check_bits(v, u, f"{what}: output {i} of the second run against the first")
    return a


def rec(name, ratio):
    RATIOS[name] = max(RATIOS[name], ratio)


def bits(name, got, ref, what=""):
    rec(name, S.check_bits(got, ref, f"{name} {what}"))


def near(name, got, ref, bnd, what=""):
    rec(name, S.check_elements(got, ref, bnd, f"{name} {what}"))


def ids(c):
    return "-".join(f"{k}={v}" for k, v in c.items() if k != "seed")


def cases(name):
    return pytest.mark.parametrize("c", R.CASES[name], ids=ids)


class Spy:
    """records the calls of ops.<name> made while the tape runs, and passes them on"""

    def __init__(self, monkeypatch, ops, name):
        self.calls, real = [], getattr(ops, name)

        def wrapper(*a, **kw):
            self.calls.append((a, kw))
            return real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)


def backward_of(tape, seeds):
    for y, dy in seeds:
        tape.accumulate(y, dy)
    return tape.backward()


# ====================================================================================================== A. GEMM
@cases("gemm_dx")
def test_gemm_data_gradient(ops, c):
    a, w, dy = R.gemm_operands(c)
    ref, ap = R.gemm_dx(dy, w)
    ad, wd, dyd = dv(a), dv(w), dv(dy)

    def run():
        tape = Tape()
        tape.require(ad)
        with tape.recording():
            y = ops.gemm(ad, wd)
        backward_of(tape, [(y, dyd)])
        assert tape.grad(wd) is None
        return cpu(tape.grad(ad))
    near("gemm dX", twice(run, "gemm dX"), ref, R.launch_bound(ref, ap))


@cases("gemm_split")
def test_gemm_two_source_split(ops, c):
    K1, K2, needs = c["K1"], c["K2"], c["needs"]
    a12, w, dy = R.gemm_operands(c, K=K1 + K2)
    ref, ap = R.gemm_dx(dy, w)
    bnd = R.launch_bound(ref, ap)
    a1d, a2d, wd, dyd = dv(a12[:, :K1].contiguous()), dv(a12[:, K1:].contiguous()), dv(w), dv(dy)

    def run():
        tape = Tape()
        if needs in ("a", "both"):
            tape.require(a1d)
        if needs in ("a2", "both"):
            tape.require(a2d)
        with tape.recording():
            y = ops.gemm(a1d, wd, a2=a2d)
        backward_of(tape, [(y, dyd)])
        return cpu(tape.grad(a1d)), cpu(tape.grad(a2d))
    g1, g2 = twice(run, "gemm split")
    assert (g1 is not None) == (needs != "a2") and (g2 is not None) == (needs != "a"), "a tensor that needs no gradient got one (or the reverse)"
    if g1 is not None:
        near("gemm dX, K split (a)", g1, ref[:, :K1], bnd[:, :K1])
    if g2 is not None:
        near("gemm dX, K split (a2)", g2, ref[:, K1:], bnd[:, K1:])


def test_gemm_residual_gradient_is_dy_itself(ops):
    c = dict(M=7, N=72, K=40, seed=1190)
    a, w, dy = R.gemm_operands(c)
    res = R.rnd(R.gen(1191), 7, 72)
    ad, wd, dyd, rd = dv(a), dv(w), dv(dy), dv(res)
    keep = dyd.clone()
    tape = Tape()
    tape.require(rd)
    with tape.recording():
        y = ops.gemm(ad, wd, residual=rd)
    backward_of(tape, [(y, dyd)])
    assert tape.grad(rd).data_ptr() == dyd.data_ptr() and tape.grad(ad) is None
    bits("gemm residual", cpu(dyd), cpu(keep), "dy after the backward")
    assert dyd.data_ptr() not in tape.owned


@cases("gemm_fanout")
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_gemm_fanout_routes(ops, monkeypatch, c, fused):
    """a feeds three GEMMs.  The backward runs them last to first: the first gradient is stored by reference (not the tape's to write), the
    second sums out of place into a buffer of the tape's own, the third is added in the GEMM's epilogue (`into`) — or, with
    AE_TAPE_FUSE_ADD=0 (autodiff.FUSE_ACCUMULATE, read once at import), by ae_add_bf16 in place."""
    from anyedit_amd import autodiff
    monkeypatch.setattr(autodiff, "FUSE_ACCUMULATE", fused)
    adds = Spy(monkeypatch, ops, "add")
    g = R.gen(c["seed"])
    M, N, K = c["M"], c["N"], c["K"]
    a = R.rnd(g, M, K)
    ws = [R.rnd(g, N, K, scale=K ** -0.5) for _ in range(3)]
    dys = [R.rnd(g, M, N) for _ in range(3)]
    pairs = [R.gemm_dx(dy, w) for dy, w in zip(dys, ws)]
    total, bnd = R.fanout_bounds([p[0] for p in pairs], [p[1] for p in pairs], fused)
    ad, wds, dyds = dv(a), [dv(w) for w in ws], [dv(dy) for dy in dys]

    def run():
        tape = Tape()
        tape.require(ad)
        seen = []

        def probe():
            cur = tape.grad(ad)
            seen.append((cur.data_ptr(), cur.data_ptr() in tape.owned, cpu(cur)))
        with tape.recording():
            ys = [ops.gemm(ad, wd) for wd in wds]
        n1, n2, n3 = tape.nodes
        tape.nodes = [n1, probe, n2, probe, n3]          # the backward runs n3, probe, n2, probe, n1
        n_add = len(adds.calls)
        backward_of(tape, list(zip(ys, dyds)))
        n_add = len(adds.calls) - n_add
        (p3, own3, g3), (p2, own2, _) = seen
        final = tape.grad(ad)
        assert not own3, "the first gradient is stored by reference: not the tape's to write"
        assert own2 and p2 != p3, "the second contribution sums out of place into a buffer of the tape's own"
        assert final.data_ptr() == p2 and p2 in tape.owned, "the third contribution is added in place to the tape's own buffer"
        assert n_add == (1 if fused else 2), f"{n_add} ae_add_bf16 launches"
        return cpu(final), g3
    got, g3 = twice(run, "fan-out")
    near("gemm dX", g3, pairs[2][0], R.launch_bound(*pairs[2]), "first of the fan-out")
    near("gemm dX, fan-out of three (into)" if fused else "gemm dX, fan-out of three (add)", got, total, bnd)


@cases("gemm_dw")
def test_gemm_parameter_gradients(ops, c):
    M, N, K = c["M"], c["N"], c["K"]
    a, w, dy = R.gemm_operands(c)
    bias = torch.randn(N, generator=R.gen(c["seed"] + 1)) * 0.1
    rw, pw = R.gemm_dw(dy, a)
    rb, pb = R.gemm_db(dy)
    with_a = (M, N) == (7, 72)
    ad, wd, bd, dyd = dv(a), dv(w), dv(bias, F32), dv(dy)

    def run():
        tape = Tape()
        tape.mark_trainable(wd, "w")
        tape.mark_trainable(bd, "b")
        if with_a:
            tape.require(ad)
        with tape.recording():
            y = ops.gemm(ad, wd, bd)
        pg = backward_of(tape, [(y, dyd)])
        assert sorted(pg) == ["b", "w"]
        assert (tape.grad(ad) is not None) == with_a
        return cpu(pg["w"]), cpu(pg["b"]), cpu(tape.grad(ad))
    gw, gb, ga = twice(run, "gemm dW")
    assert gw.dtype == F32 and gb.dtype == F32
    near("gemm dW", gw, rw, R.launch_bound(rw, pw, f32=True))
    near("gemm db", gb, rb, R.launch_bound(rb, pb, f32=True))
    if with_a:
        rx, px = R.gemm_dx(dy, w)
        near("gemm dX", ga, rx, R.launch_bound(rx, px), "next to a trainable weight")


@pytest.mark.parametrize("M", [7, 33])
def test_two_gemms_share_a_trainable_weight(ops, M):
    c = dict(M=M, N=72, K=40, seed=1390 + M)
    a1, w, dy1 = R.gemm_operands(c)
    g = R.gen(c["seed"] + 50)
    a2, dy2 = R.rnd(g, M, 40), R.rnd(g, M, 72)
    (r1, p1), (r2, p2) = R.gemm_dw(dy1, a1), R.gemm_dw(dy2, a2)
    tot, bnd = R.sum_of_launches([r1, r2], [p1, p2])
    a1d, a2d, wd, d1, d2 = dv(a1), dv(a2), dv(w), dv(dy1), dv(dy2)

    def run():
        tape = Tape()
        tape.mark_trainable(wd, "w")
        with tape.recording():
            y1, y2 = ops.gemm(a1d, wd), ops.gemm(a2d, wd)
        return cpu(backward_of(tape, [(y1, d1), (y2, d2)])["w"])
    near("gemm dW, weight used twice", twice(run, "shared weight"), tot, bnd)


# ====================================================================================================== A. conv
def conv_run(ops, c, x, w, dy, stride=1, up=False, **kw):
    """one conv node on a tape -> dX on the CPU"""
    B, H, W = c["B"], c["H"], c["W"]
    xd, wp, dyd = dv(x), ops.pack_conv3x3(dv(w, F32)), dy if dy.is_cuda else dv(dy)

    def run():
        tape = Tape()
        tape.require(xd)
        with tape.recording():
            y, Ho, Wo = ops.conv3x3(xd, wp, kw.get("bias"), B, H, W, addvec=kw.get("addvec"), stride=stride, upsample2x=up, out_f32=kw.get("out_f32", False))
        assert (Ho, Wo) == R.conv_out_hw(H, W, stride, up)
        backward_of(tape, [(y, dyd)])
        return cpu(tape.grad(xd))
    return twice(run, "conv dX")


@cases("conv_s1")
def test_conv_stride1(ops, c):
    x, w, dy = R.conv_operands(c)
    ref, ap = R.conv_dx(dy, w, c["B"], c["H"], c["W"])
    near("conv dX, stride 1", conv_run(ops, c, x, w, dy), ref, R.launch_bound(ref, ap))


def test_conv_residual_bias_addvec_and_fp32_output(ops):
    c = dict(B=2, H=3, W=5, Cin=72, Cout=136, seed=1490)
    B, H, W, Cout = c["B"], c["H"], c["W"], c["Cout"]
    x, w, dy = R.conv_operands(c)
    ref, ap = R.conv_dx(dy, w, B, H, W)
    plain = conv_run(ops, c, x, w, dy)
    # bias and addvec present, neither needing a gradient: the same launches on the same operands
    g = R.gen(1491)
    bias, addvec = dv(torch.randn(Cout, generator=g), F32), dv(torch.randn(B, Cout, generator=g), F32)
    bits("conv dX, stride 1", conv_run(ops, c, x, w, dy, bias=bias, addvec=addvec), plain, "with bias and addvec against without")
    # fp32 output: the gradient arrives in fp32 and is rounded to bf16 once
    dy32 = torch.randn(B * H * W, Cout, generator=g)
    r32, a32 = R.conv_dx(R.q(dy32), w, B, H, W)
    near("conv dX, stride 1", conv_run(ops, c, x, w, dy32.to(DEV), out_f32=True), r32, R.launch_bound(r32, a32), "fp32 output")
    # a residual that needs a gradient: it is dy itself
    xd, wp, dyd, rd = dv(x), ops.pack_conv3x3(dv(w, F32)), dv(dy), dv(R.rnd(g, B * H * W, Cout))
    keep = dyd.clone()
    tape = Tape()
    tape.require(xd)
    tape.require(rd)
    with tape.recording():
        y, _, _ = ops.conv3x3(xd, wp, None, B, H, W, residual=rd)
    backward_of(tape, [(y, dyd)])
    assert tape.grad(rd).data_ptr() == dyd.data_ptr()
    bits("conv residual", cpu(dyd), cpu(keep), "dy after the backward")
    near("conv dX, stride 1", cpu(tape.grad(xd)), ref, R.launch_bound(ref, ap), "with a residual")


@cases("conv_up")
def test_conv_nearest_up(ops, c):
    x, w, dy = R.conv_operands(c, up=True)
    ref, bnd = R.conv_up_dx(dy, w, c["B"], c["H"], c["W"])
    near("conv dX, nearest x2 (+ 2x2 sums)", conv_run(ops, c, x, w, dy, up=True), ref, bnd)


@cases("conv_s2")
def test_conv_stride2(ops, c):
    x, w, dy = R.conv_operands(c, stride=2)
    ref, ap = R.conv_dx(dy, w, c["B"], c["H"], c["W"], stride=2)
    odd = c["H"] % 2 or c["W"] % 2
    near("conv dX, stride 2, odd map (crop)" if odd else "conv dX, stride 2, even map", conv_run(ops, c, x, w, dy, stride=2), ref, R.launch_bound(ref, ap))


def test_even_stride2_maps_launch_what_they_did(ops, monkeypatch):
    """no copy on an even map: the gradient is the adjoint conv's own output buffer"""
    c = dict(B=2, H=4, W=6, Cin=8, Cout=72, seed=1690)
    x, w, dy = R.conv_operands(c, stride=2)
    xd, wp, dyd = dv(x), ops.pack_conv3x3(dv(w, F32)), dv(dy)
    tape = Tape()
    tape.require(xd)
    with tape.recording():
        y, _, _ = ops.conv3x3(xd, wp, None, 2, 4, 6, stride=2)
    outs, real = [], ops.conv3x3

    def keep_out(*a, **kw):
        r = real(*a, **kw)
        outs.append((r[0], kw))
        return r
    monkeypatch.setattr(ops, "conv3x3", keep_out)
    backward_of(tape, [(y, dyd)])
    assert len(outs) == 1 and outs[0][1].get("upsample2x") == 2, "one zero-insert conv launch"
    assert tape.grad(xd).data_ptr() == outs[0][0].data_ptr(), "the gradient is the launch's own output: no copy"


# ====================================================================================================== A. weight caches
def test_weight_caches(ops):
    from anyedit_amd import autodiff
    c = dict(M=7, N=72, K=40, seed=1900)
    a, w, dy = R.gemm_operands(c)
    ad, dyd = dv(a), dv(dy)

    def gemm_tape(wd):
        tape = Tape()
        tape.require(ad)
        with tape.recording():
            y = ops.gemm(ad, wd)
        backward_of(tape, [(y, dyd)])
        return tape, cpu(tape.grad(ad))
    wd = dv(w)
    t1, g1 = gemm_tape(wd)
    ent = autodiff._FROZEN_WT[id(wd)]
    assert ent[0] is wd, "the cache keeps the key tensor alive (its id stays unique)"
    t2, g2 = gemm_tape(wd)
    assert autodiff._FROZEN_WT[id(wd)] is ent and t1.transposed(wd) is t2.transposed(wd), "built once"
    bits("weight cache (transposed)", cpu(ent[1]), cpu(wd.t().contiguous()))
    bits("weight cache (transposed)", g2, g1, "second tape")
    del wd
    w2 = R.rnd(R.gen(1901), 72, 40, scale=40 ** -0.5)
    w2d = dv(w2)                                   # allocated after the first was released by the test: the cache still holds the first
    assert w2d.data_ptr() != ent[0].data_ptr() and id(w2d) != id(ent[0])
    _, g3 = gemm_tape(w2d)
    assert autodiff._FROZEN_WT[id(w2d)][0] is w2d
    r3, p3 = R.gemm_dx(dy, w2)
    near("gemm dX", g3, r3, R.launch_bound(r3, p3), "a second frozen weight")
    # a trainable weight is cached per tape only
    tape = Tape()
    tape.mark_trainable(w2d, "w")
    before = len(autodiff._FROZEN_WT)
    assert tape.transposed(w2d) is tape.transposed(w2d) and len(autodiff._FROZEN_WT) == before
    # rotated conv weights
    cc = dict(B=2, H=3, W=5, Cin=8, Cout=64, seed=1902)
    x, wc, dyc = R.conv_operands(cc)
    wp = ops.pack_conv3x3(dv(wc, F32))
    ta, tb = Tape(), Tape()
    ra = ta.rotated(wp, 8)
    assert tb.rotated(wp, 8) is ra and autodiff._FROZEN_WROT[id(wp)][0] is wp
    assert tuple(ra.shape) == (8, 9 * 64)
    wp2 = ops.pack_conv3x3(dv(R.rnd(R.gen(1903), 64, 8, 3, 3), F32))
    assert ta.rotated(wp2, 8) is not ra and autodiff._FROZEN_WROT[id(wp2)][0] is wp2
    # w'[ci][ky'][kx'][co] = w[co][2-ky'][2-kx'][ci], zero beyond Cout
    want = torch.zeros(8, 3, 3, 64, dtype=F64)
    want[..., :64] = wc.flip(2, 3).permute(1, 2, 3, 0)
    bits("weight cache (rotated)", cpu(ra), want.reshape(8, 9 * 64).to(BF))


# ====================================================================================================== B. layout adjoints
@cases("concat")
def test_concat_adjoint_routes(ops, monkeypatch, c):
    g = R.gen(c["seed"])
    rows, ca, cb = c["rows"], c["ca"], c["cb"]
    a, b, dy = R.rnd(g, rows, ca), R.rnd(g, rows, cb), R.rnd(g, rows, ca + cb)
    o1, o2, base = R.rnd(g, rows, ca), R.rnd(g, rows, ca), R.rnd(g, 2 * rows, max(ca, cb))
    ad, bd, dyd, o1d, o2d, based = dv(a), dv(b), dv(dy), dv(o1), dv(o2), dv(base)
    sa, sb = dy[:, :ca].to(BF).contiguous(), dy[:, ca:].to(BF).contiguous()
    splits = Spy(monkeypatch, ops, "split_channels")

    def run(mode):
        def go():
            tape = Tape()
            xa, xb = ad, bd
            if mode == "views":                       # a and b are views of one base: the two-launch route, no gradient for a partial view
                xa, xb = based[:rows, :ca], based[rows:, :cb]
            if mode != "only_b":
                tape.require(xa)
            if mode != "only_a":
                tape.require(xb)
            with tape.recording():
                y = ops.concat_channels(xa, xb)
            if mode == "owned":                       # two contributions: the sum is a buffer of the tape's own
                tape.accumulate(xa, o1d)
                tape.accumulate(xa, o2d)
                assert tape.grad(xa).data_ptr() in tape.owned
            if mode == "borrowed":
                tape.accumulate(xa, o1d)
                assert tape.grad(xa).data_ptr() == o1d.data_ptr()
            n = len(splits.calls)
            if mode == "views":
                with pytest.raises(RuntimeError, match="partial view"):
                    backward_of(tape, [(y, dyd)])
                return None, None, 0
            backward_of(tape, [(y, dyd)])
            ga, gb = tape.grad(xa), tape.grad(xb)
            if mode in ("fresh", "owned"):
                assert ga.data_ptr() in tape.owned and gb.data_ptr() in tape.owned, "the buffers the split wrote are the tape's own"
            return cpu(ga), cpu(gb), len(splits.calls) - n
        return twice(lambda: go()[:2], f"concat {mode}") + (go()[2],)

    ga, gb, n = run("fresh")
    assert n == 1, "both gradients fresh: one ae_split_channels_bf16 launch"
    bits("concat adjoint", ga, sa, "fresh a")
    bits("concat adjoint", gb, sb, "fresh b")
    ga, gb, n = run("owned")
    assert n == 1, "an owned gradient is added to in the same launch"
    old = R.q(o1 + o2)
    ref, bnd = R.concat_add(old, dy[:, :ca])
    near("concat adjoint (added in place)", ga, ref, bnd)
    bits("concat adjoint", gb, sb, "b next to an owned a")
    keep = o1d.clone()
    ga, gb, n = run("borrowed")
    assert n == 0, "a borrowed gradient is never written: the two-launch route"
    bits("concat adjoint", cpu(o1d), cpu(keep), "the borrowed gradient after the backward")
    ref, bnd = R.concat_add(o1, dy[:, :ca])
    near("concat adjoint (added out of place)", ga, ref, bnd)
    bits("concat adjoint", gb, sb, "b next to a borrowed a")
    ga, gb, n = run("only_a")
    assert gb is None
    bits("concat adjoint", ga, sa, "only a")
    ga, gb, n = run("only_b")
    assert ga is None
    bits("concat adjoint", gb, sb, "only b")
    run("views")


def test_concat_of_two_whole_views_of_one_base(ops):
    """a and b are reshaped views of ONE base tensor: both halves are gradients of that base and must be summed, not overwritten"""
    g = R.gen(1790)
    rows, ch = 7, 8
    base, dy = R.rnd(g, rows, ch), R.rnd(g, rows, 2 * ch)
    based, dyd = dv(base), dv(dy)

    def run():
        tape = Tape()
        tape.require(based)
        xa, xb = based.view(rows, ch), based.view(rows, ch)
        with tape.recording():
            y = ops.concat_channels(xa, xb)
        backward_of(tape, [(y, dyd)])
        return cpu(tape.grad(based))
    ref, bnd = R.concat_add(dy[:, :ch], dy[:, ch:])
    near("concat adjoint (one base)", twice(run, "concat one base"), ref, bnd)


@cases("rows_to_nchw")
def test_rows_to_nchw_adjoint(ops, c):
    g = R.gen(c["seed"])
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    x = R.rnd(g, B * H * W, C)
    dy = torch.randn(B, C, H, W, generator=g)
    odt = BF if c["bf16"] else F32
    dy = dy.to(odt)
    xd, dyd = dv(x), dy.to(DEV)

    def run():
        tape = Tape()
        tape.require(xd)
        with tape.recording():
            y = ops.rows_to_nchw(xd, B, H, W, out_dtype=odt)
        assert y.dtype == odt and tuple(y.shape) == (B, C, H, W)
        bits("rows_to_nchw forward", cpu(y), R.to_nchw(x, B, H, W).to(odt).contiguous())
        backward_of(tape, [(y, dyd)])
        return cpu(tape.grad(xd))
    bits("rows_to_nchw adjoint", twice(run, "rows_to_nchw"), R.nchw_adjoint(dy.to(F64)).contiguous())


# ====================================================================================================== C. GroupNorm
@pytest.mark.parametrize("HW", [6, 257])
@pytest.mark.parametrize("two,silu", [(False, False), (False, True), (True, False), (True, True)], ids=["x", "x-silu", "x-x2", "x-x2-silu"])
def test_groupnorm_routing(ops, monkeypatch, HW, two, silu):
    g = R.gen(2000 + HW + 2 * two + silu)
    B, C, C1, eps = 2, 64, 24, 1e-5
    xall = NR.make_x(g, B, HW, C, 32).reshape(B * HW, C)
    gamma, beta = NR.make_affine(g, C)
    c1 = C1 if two else C
    xd, x2d = xall[:, :c1].contiguous().to(DEV), (xall[:, c1:].contiguous().to(DEV) if two else None)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    dyd, o1, o2 = (dv(R.rnd(g, B * HW, C)) for _ in range(3))
    p1, p2 = dv(R.rnd(g, B * HW, c1)), dv(R.rnd(g, B * HW, c1))
    q1, q2 = (dv(R.rnd(g, B * HW, C - c1)), dv(R.rnd(g, B * HW, C - c1))) if two else (None, None)
    # the direct call: the forward's statistics, then the wrapper the tape calls
    stat = torch.empty(B, 32, 2, dtype=F32, device=DEV)
    y_direct = ops.groupnorm(xd, gd, bd, B, HW, eps, silu=silu, x2=x2d, stat_out=stat)

    def direct(dx_into=None, dx2_into=None):
        return ops.groupnorm_bwd(xd, gd, bd, dyd, B, HW, eps, silu=silu, groups=32, x2=x2d, stat=stat, dx_into=dx_into, dx2_into=dx2_into)
    spy = Spy(monkeypatch, ops, "groupnorm_bwd")

    def run(mode):
        def go():
            tape = Tape()
            tape.require(xd)
            if two:
                tape.require(x2d)
            with tape.recording():
                y = ops.groupnorm(xd, gd, bd, B, HW, eps, silu=silu, x2=x2d)
            bits("groupnorm forward", cpu(y), cpu(y_direct))
            if mode in ("owned", "owned_x2"):
                t, (u, v) = (xd, (p1, p2)) if mode == "owned" else (x2d, (q1, q2))
                tape.accumulate(t, u)
                tape.accumulate(t, v)
            if mode == "borrowed":
                tape.accumulate(xd, p1)
            n = len(spy.calls)
            backward_of(tape, [(y, dyd)])
            assert len(spy.calls) == n + 1
            kw = spy.calls[-1][1]
            bits("groupnorm statistics", cpu(kw["stat"]), cpu(stat), "the forward's statistics reach the backward")
            return cpu(tape.grad(xd)), cpu(tape.grad(x2d)) if two else None, kw["dx_into"] is not None, kw["dx2_into"] is not None
        r = twice(lambda: go()[:2], f"groupnorm {mode}")
        return r + go()[2:]

    dx, dx2 = direct()
    gx, gx2, into1, into2 = run("fresh")
    assert not into1 and not into2
    bits("groupnorm (tape = direct call)", gx, cpu(dx))
    if two:
        bits("groupnorm (tape = direct call)", gx2, cpu(dx2))
    # x already has a gradient of the tape's own: added in the kernel
    own = ops.add(p1, p2)
    want, _ = direct(dx_into=own.clone())
    gx, gx2, into1, into2 = run("owned")
    assert into1 and not into2, "dx_into exactly when x has an owned gradient"
    bits("groupnorm (tape = direct call)", gx, cpu(want), "dx_into")
    if two:
        bits("groupnorm (tape = direct call)", gx2, cpu(dx2), "dx2 next to dx_into")
        own2 = ops.add(q1, q2)
        _, want2 = direct(dx2_into=own2.clone())
        gx, gx2, into1, into2 = run("owned_x2")
        assert into2 and not into1, "dx2_into exactly when x2 has an owned gradient"
        bits("groupnorm (tape = direct call)", gx2, cpu(want2), "dx2_into")
        bits("groupnorm (tape = direct call)", gx, cpu(dx), "dx next to dx2_into")
    # a borrowed gradient is never written: out of place
    keep = p1.clone()
    gx, gx2, into1, into2 = run("borrowed")
    assert not into1 and not into2, "never into a borrowed gradient"
    bits("groupnorm (tape = direct call)", cpu(p1), cpu(keep), "the borrowed gradient after the backward")
    bits("groupnorm (tape = direct call)", gx, cpu(ops.add(p1, dx)), "borrowed + dx")


def test_groupnorm_never_adds_into_its_own_dy(ops, monkeypatch):
    """x's gradient and y's gradient are ONE buffer of the tape's own (x reached y's consumer as a residual, stored by reference): the kernel
    must not be handed it as dx_into while it reads it as dy"""
    g = R.gen(2090)
    B, HW, C, eps = 2, 6, 64, 1e-5
    xd = NR.make_x(g, B, HW, C, 32).reshape(B * HW, C).to(DEV)
    gamma, beta = NR.make_affine(g, C)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    d1, d2 = dv(R.rnd(g, B * HW, C)), dv(R.rnd(g, B * HW, C))
    tape = Tape()
    tape.require(xd)
    with tape.recording():
        y = ops.groupnorm(xd, gd, bd, B, HW, eps)
    tape.accumulate(y, d1)
    tape.accumulate(y, d2)
    dy = tape.grad(y)
    assert dy.data_ptr() in tape.owned
    tape.accumulate(xd, dy)
    assert tape.grad(xd).data_ptr() == dy.data_ptr()
    dy_keep = dy.clone()
    dx, _ = ops.groupnorm_bwd(xd, gd, bd, dy_keep, B, HW, eps)
    spy = Spy(monkeypatch, ops, "groupnorm_bwd")
    tape.backward()
    assert len(spy.calls) == 1 and spy.calls[0][1]["dx_into"] is None, "dx_into aliases dy"
    bits("groupnorm (tape = direct call)", cpu(tape.grad(xd)), cpu(ops.add(dy_keep, dx)), "dy + dx")


# ====================================================================================================== C. LayerNorm, GEGLU
@pytest.mark.parametrize("M,C", [(1, 64), (10, 64), (1, 1032), (10, 1032)])
@pytest.mark.parametrize("train", ["none", "gamma", "beta", "both"])
def test_layernorm_routing(ops, monkeypatch, M, C, train):
    g = R.gen(2100 + M + C)
    xd = NR.make_x(g, M, 1, C, 1, const_group=False).reshape(M, C).to(DEV)
    gamma, beta = NR.make_affine(g, C)
    gd, bd, dyd = gamma.to(DEV), beta.to(DEV), dv(R.rnd(g, M, C))
    p1, p2 = dv(R.rnd(g, M, C)), dv(R.rnd(g, M, C))
    want_pg = train != "none"
    dx, dg, db = ops.layernorm_bwd(xd, gd, dyd, 1e-5, want_param_grads=want_pg)
    y_direct = ops.layernorm(xd, gd, bd, 1e-5)
    spy = Spy(monkeypatch, ops, "layernorm_bwd")

    def run(owned, need_x=True):
        def go():
            tape = Tape()
            if need_x:
                tape.require(xd)
            if train in ("gamma", "both"):
                tape.mark_trainable(gd, "ln.gamma")
            if train in ("beta", "both"):
                tape.mark_trainable(bd, "ln.beta")
            with tape.recording():
                y = ops.layernorm(xd, gd, bd, 1e-5)
            bits("layernorm forward", cpu(y), cpu(y_direct))
            if not need_x and not want_pg:
                assert not tape.nodes and not tape.needs(y), "nothing needs a gradient: no node"
                return None, None, None, False
            if owned:
                tape.accumulate(xd, p1)
                tape.accumulate(xd, p2)
            n = len(spy.calls)
            pg = backward_of(tape, [(y, dyd)])
            assert len(spy.calls) == n + 1
            assert sorted(pg) == sorted(nm for nm, on in (("ln.gamma", train in ("gamma", "both")), ("ln.beta", train in ("beta", "both"))) if on)
            return cpu(tape.grad(xd)), cpu(pg.get("ln.gamma")), cpu(pg.get("ln.beta")), spy.calls[-1][1]["dx_into"] is not None
        return twice(lambda: go()[:3], "layernorm") + go()[3:]

    gx, gg, gb, into = run(False)
    assert not into
    bits("layernorm (tape = direct call)", gx, cpu(dx))
    if gg is not None:
        bits("layernorm (tape = direct call)", gg, cpu(dg), "dgamma under its name")
    if gb is not None:
        bits("layernorm (tape = direct call)", gb, cpu(db), "dbeta under its name")
    want, _, _ = ops.layernorm_bwd(xd, gd, dyd, 1e-5, want_param_grads=want_pg, dx_into=ops.add(p1, p2))
    gx, _, _, into = run(True)
    assert into
    bits("layernorm (tape = direct call)", gx, cpu(want), "dx_into")
    gx, gg, gb, into = run(False, need_x=False)
    assert gx is None and not into
    if gg is not None:
        bits("layernorm (tape = direct call)", gg, cpu(dg), "dgamma without dx")


def test_geglu_routing(ops):
    g = R.gen(2200)
    h, dy = R.rnd(g, 7, 144), R.rnd(g, 7, 72)
    hd, dyd = dv(h), dv(dy)
    want = ops.geglu_bwd(hd, dyd)

    def run():
        tape = Tape()
        tape.require(hd)
        with tape.recording():
            y = ops.geglu(hd)
        backward_of(tape, [(y, dyd)])
        return cpu(tape.grad(hd))
    got = twice(run, "geglu")
    bits("geglu (tape = direct call)", got, cpu(want))
    ref, bnd = S.ref_geglu_bwd(h, dy)
    near("geglu against float64", got, ref, bnd)


# ====================================================================================================== C. attention
ATTN_B, ATTN_H = 2, 3


class Attn:
    """operands of one attention problem in the tape's layouts: fused `qkv` rows, or query rows and a packed key/value base that is 8
    columns wider than its views"""

    def __init__(self, D, Nq, Nk, fused, seed, pad=8):
        g = R.gen(seed)
        B, H = ATTN_B, ATTN_H
        C = self.C = H * D
        self.D, self.Nq, self.Nk, self.scale = D, Nq, Nk, D ** -0.5
        if fused:
            self.base = dv(R.rnd(g, B * Nq, 3 * C))
            self.q, self.k, self.v = self.base[:, :C], self.base[:, C:2 * C], self.base[:, 2 * C:]
            self.qs = self.ks = (Nq * 3 * C, D, 3 * C)
        else:
            self.q = dv(R.rnd(g, B * Nq, C))
            self.base = dv(R.rnd(g, B * Nk, 2 * C + pad))
            self.k, self.v = self.base[:, :C], self.base[:, C:2 * C]
            self.qs, self.ks = (Nq * C, D, C), (Nk * (2 * C + pad), D, 2 * C + pad)
        self.dy = dv(R.rnd(g, B, Nq, C))
        self.dims = (B, H, Nq, Nk, D, self.scale)

    def forward(self, ops, **kw):
        return ops.attention(self.q, self.k, self.v, *self.dims, self.qs, self.ks, self.ks, **kw)

    def heads(self, t, n):
        """[B*n, >= C] view -> float64 [B, H, n, D]"""
        return t.detach().cpu().to(F64).reshape(ATTN_B, n, ATTN_H, self.D).permute(0, 2, 1, 3)


def zero_views(*tensors):
    """a zero-filled gradient buffer per distinct base, and per-tensor views at the forward's offsets"""
    bufs, views = {}, []
    for t in tensors:
        b = t._base if t._base is not None else t
        if id(b) not in bufs:
            bufs[id(b)] = torch.zeros_like(b)
        views.append(bufs[id(b)].as_strided(t.shape, t.stride(), t.storage_offset() - b.storage_offset()))
    return list(bufs.values()), views


def poison_allocator(like):
    """leave NaN patterns in the block the allocator is likely to hand out next for a tensor like `like`"""
    t = torch.empty_like(like)
    t.view(torch.int16).fill_(0x7FA5)
    del t


@pytest.mark.parametrize("D", [40, 64])
@pytest.mark.parametrize("N", [33, 130])
def test_attention_fused_qkv_base(ops, monkeypatch, D, N):
    P = Attn(D, N, N, True, 2300 + D + N)
    lse = torch.empty(ATTN_B, ATTN_H, N, dtype=F32, device=DEV)
    y_direct = P.forward(ops, lse=lse)
    (gbuf,), (dq, dk, dv_) = zero_views(P.q, P.k, P.v)
    ops.attention_bwd(P.q, P.k, P.v, P.dy, lse, *P.dims, P.qs, P.ks, P.ks, dq, dk, dv_, P.qs, P.ks, P.ks, out=y_direct)
    zeros = Spy(monkeypatch, torch.Tensor, "zero_")
    spy = Spy(monkeypatch, ops, "attention_bwd")

    def run():
        tape = Tape()
        tape.require(P.base)
        with tape.recording():
            y = P.forward(ops)
        bits("attention forward", cpu(y), cpu(y_direct))
        tape.accumulate(y, P.dy)
        poison_allocator(P.base)
        nz = len(zeros.calls)
        tape.backward()
        assert len(zeros.calls) == nz, "a fully covered buffer is not zero-filled"
        assert spy.calls[-1][1]["out"] is y, "the segment's own output goes to the backward"
        got = tape.grad(P.base)
        assert bool(torch.isfinite(got).all()), "the three views do not cover the fused gradient buffer"
        return cpu(got)
    bits("attention, fused qkv (tape = direct call)", twice(run, "fused qkv"), cpu(gbuf))


@pytest.mark.parametrize("D", [40, 64])
@pytest.mark.parametrize("Nq,Nk", [(33, 1), (33, 77), (130, 1), (130, 77)])
def test_attention_query_rows_and_packed_kv_base(ops, monkeypatch, D, Nq, Nk):
    P = Attn(D, Nq, Nk, False, 2400 + D + Nq + Nk)
    C = P.C
    lse = torch.empty(ATTN_B, ATTN_H, Nq, dtype=F32, device=DEV)
    y_direct = P.forward(ops, lse=lse)
    (gq, gkv), (dq, dk, dv_) = zero_views(P.q, P.k, P.v)
    ops.attention_bwd(P.q, P.k, P.v, P.dy, lse, *P.dims, P.qs, P.ks, P.ks, dq, dk, dv_, P.qs, P.ks, P.ks, out=y_direct)
    (gq_only,), (dq1,) = zero_views(P.q)
    ops.attention_bwd(P.q, P.k, P.v, P.dy, lse, *P.dims, P.qs, P.ks, P.ks, dq1, None, None, P.qs, P.ks, P.ks, out=y_direct)
    spy = Spy(monkeypatch, ops, "attention_bwd")

    def run(kv_too):
        def go():
            tape = Tape()
            tape.require(P.q)
            if kv_too:
                tape.require(P.base)
            with tape.recording():
                y = P.forward(ops)
            tape.accumulate(y, P.dy)
            poison_allocator(P.base)
            tape.backward()
            a = spy.calls[-1][0]
            assert (a[15] is not None) == kv_too and (a[16] is not None) == kv_too, "dk / dv exactly when the key/value side needs a gradient"
            return cpu(tape.grad(P.q)), cpu(tape.grad(P.base))
        return twice(go, "q + packed kv")
    got_q, got_kv = run(True)
    bits("attention, q + packed kv (tape = direct call)", got_q, cpu(gq))
    bits("attention, q + packed kv (tape = direct call)", got_kv, cpu(gkv))
    pad = got_kv[:, 2 * C:]
    assert bool((pad.view(torch.int16) == 0).all()), "the uncovered columns of the packed gradient must be exactly 0"
    got_q, got_kv = run(False)
    assert got_kv is None, "only q needs a gradient"
    bits("attention, only q (tape = direct call)", got_q, cpu(gq_only))


@pytest.mark.parametrize("D", [40, 64])
@pytest.mark.parametrize("Nq,Nk,Nk2", [(33, 77, 1), (130, 1, 77)])
@pytest.mark.parametrize("fused", [False, True], ids=["accumulate", "seg2"])
def test_attention_two_segments_and_gate(ops, monkeypatch, D, Nq, Nk, Nk2, fused):
    """out = Attn(q, K, V) + gate_b Attn(q, K2, V2), as a second call that accumulates into the first one's output (`out_scale`,
    `accumulate=True`) or as one two-segment launch (`seg2`)."""
    B, H = ATTN_B, ATTN_H
    P = Attn(D, Nq, Nk, False, 2500 + D + Nq + fused, pad=0)
    P2 = Attn(D, Nq, Nk2, False, 2600 + D + Nq + fused, pad=0)
    C = P.C
    gate = torch.tensor([0.7, -0.3], dtype=F32, device=DEV)
    dims2 = (B, H, Nq, Nk2, D, P.scale)
    l1, l2 = (torch.empty(B, H, Nq, dtype=F32, device=DEV) for _ in range(2))
    # the direct calls
    if fused:
        y_direct = P.forward(ops, seg2=(P2.k, P2.v, Nk2, P2.ks, P2.ks, gate), lse=l1, lse2=l2)
    else:
        y_direct = P.forward(ops, lse=l1)
        first_alone = y_direct.clone()
        ops.attention(P.q, P2.k, P2.v, *dims2, P.qs, P2.ks, P2.ks, out=y_direct, out_scale=gate, accumulate=True, lse=l2)
    (gq1, gkv1), (dq, dk, dv_) = zero_views(P.q, P.k, P.v)
    (gkv2,), (dk2, dv2) = zero_views(P2.k, P2.v)
    ops.attention_bwd(P.q, P.k, P.v, P.dy, l1, *P.dims, P.qs, P.ks, P.ks, dq, dk, dv_, P.qs, P.ks, P.ks)                       # no out=: y is not one segment's
    if fused:
        delta2 = ops.attention_bwd(P.q, P2.k, P2.v, P.dy, l2, *dims2, P.qs, P2.ks, P2.ks, dq, dk2, dv2, P.qs, P2.ks, P2.ks, out_scale=gate, accumulate_dq=True)
        want_q = gq1
    else:
        (gq2,), (dq2,) = zero_views(P.q)
        delta2 = ops.attention_bwd(P.q, P2.k, P2.v, P.dy, l2, *dims2, P.qs, P2.ks, P2.ks, dq2, dk2, dv2, P.qs, P2.ks, P2.ks, out_scale=gate)
        want_q = ops.add(gq2, gq1)              # the second call's node runs first: its dq is stored by reference, the first call's is added
    want_gate = ops.rowsum_f32(delta2.reshape(B, -1))
    spy = Spy(monkeypatch, ops, "attention_bwd")

    def run():
        tape = Tape()
        for t in (P.q, P.base, P2.base, gate):
            tape.require(t)
        with tape.recording():
            if fused:
                y = P.forward(ops, seg2=(P2.k, P2.v, Nk2, P2.ks, P2.ks, gate))
            else:
                y = P.forward(ops)
                bits("attention forward", cpu(y), cpu(first_alone))
                y2 = ops.attention(P.q, P2.k, P2.v, *dims2, P.qs, P2.ks, P2.ks, out=y, out_scale=gate, accumulate=True)
                assert y2 is y and id(y) in tape.mutated
        bits("attention forward", cpu(y), cpu(y_direct), "both segments")
        tape.accumulate(y, P.dy)
        n = len(spy.calls)
        tape.backward()
        assert len(spy.calls) == n + 2
        assert all(kw.get("out") is None for _, kw in spy.calls[n:]), "an output that holds two segments is never handed to the backward"
        gg = tape.grads[id(gate)]
        assert gg.dtype == F32 and tuple(gg.shape) == (B,)
        return cpu(tape.grad(P.q)), cpu(tape.grad(P.base)), cpu(tape.grad(P2.base)), cpu(gg)
    got_q, got_kv, got_kv2, got_gate = twice(run, "two segments")
    name = "attention, seg2 (tape = direct calls)" if fused else "attention, accumulate (tape = direct calls)"
    bits(name, got_q, cpu(want_q), "dq")
    bits(name, got_kv, cpu(gkv1), "first segment's dk | dv")
    bits(name, got_kv2, cpu(gkv2), "second segment's dk | dv")
    bits(name, got_gate, cpu(want_gate), "gate gradient = rowsum(delta)")
    ref, lim = R.gate_grad(R.attn_delta(P.heads(P.q, Nq), P.heads(P2.k, Nk2), P.heads(P2.v, Nk2), P.heads(P.dy.reshape(B * Nq, C), Nq), P.scale))
    near("attention gate gradient against float64", got_gate, ref, lim + 1e-30)


# ====================================================================================================== C. checkpoint
@pytest.mark.parametrize("checkpointed", [False, True], ids=["plain", "checkpoint"])
def test_checkpoint_segment(ops, checkpointed):
    """LayerNorm -> GEMM (trainable weight, residual) -> GEGLU as one segment, recorded plainly and under `Tape.checkpoint`: the same forward
    bits, and every gradient that leaves the segment (the input, the residual, the parameter) within the bound of
    tape_ref.segment_adjoint, whichever way it was recorded"""
    c = R.SEGMENT
    x, gamma, beta, w, r, dy = R.segment_operands()
    eps = c["eps"]
    xd, gd, bd, wd, rd, dyd = dv(x), gamma.to(DEV), beta.to(DEV), dv(w), dv(r), dv(dy)
    # the forward values the backward reads (the checkpointed run drops and recomputes them: same kernels, same bits)
    hd = ops.layernorm(xd, gd, bd, eps)
    ud = ops.gemm(hd, wd, residual=rd)
    y_direct = ops.geglu(ud)
    ref = R.segment_adjoint(x, gamma, beta, w, cpu(hd).to(F64), cpu(ud).to(F64), dy, eps)

    def body():
        return ops.geglu(ops.gemm(ops.layernorm(xd, gd, bd, eps), wd, residual=rd))

    def run():
        tape = Tape()
        tape.mark_trainable(wd, "w")
        tape.require(xd)
        tape.require(rd)
        with tape.recording():
            y = tape.checkpoint(body) if checkpointed else body()
        assert len(tape.nodes) == (1 if checkpointed else 3)
        bits("checkpoint forward", cpu(y), cpu(y_direct))
        pg = backward_of(tape, [(y, dyd)])
        assert sorted(pg) == ["w"]
        return cpu(tape.grad(xd)), cpu(tape.grad(rd)), cpu(pg["w"])
    dx, dr, dw = twice(run, "segment")
    tag = " (checkpointed)" if checkpointed else " (plain)"
    near("segment dx" + tag, dx, *ref["dx"])
    near("segment d residual" + tag, dr, *ref["dr"])
    near("segment dW" + tag, dw, *ref["dw"])


@pytest.mark.parametrize("checkpointed", [False, True], ids=["plain", "checkpoint"])
def test_checkpoint_hands_an_fp32_gate_gradient_across(ops, checkpointed):
    """the gate of an accumulating attention call is an fp32 leaf outside the segment: its gradient crosses the segment's border in fp32"""
    B, H, D, Nq, Nk, Nk2 = ATTN_B, ATTN_H, 40, 33, 77, 1
    P, P2 = Attn(D, Nq, Nk, False, 2700, pad=0), Attn(D, Nq, Nk2, False, 2701, pad=0)
    gate = torch.tensor([0.7, -0.3], dtype=F32, device=DEV)
    dims2 = (B, H, Nq, Nk2, D, P.scale)

    def body():
        y = P.forward(ops)
        return ops.attention(P.q, P2.k, P2.v, *dims2, P.qs, P2.ks, P2.ks, out=y, out_scale=gate, accumulate=True)

    def run():
        tape = Tape()
        for t in (P.q, P2.base, gate):
            tape.require(t)
        with tape.recording():
            y = tape.checkpoint(body) if checkpointed else body()
        backward_of(tape, [(y, P.dy)])
        gg = tape.grads[id(gate)]
        assert gg.dtype == F32 and tape.grad(P.base) is None
        return cpu(y), cpu(gg), cpu(tape.grad(P.q)), cpu(tape.grad(P2.base))
    y_direct = cpu(body())
    y, gg, gq, gkv2 = twice(run, "gate across a checkpoint")
    bits("checkpoint forward", y, y_direct, "attention segment")
    assert bool(torch.isfinite(gq.float()).all()) and bool(torch.isfinite(gkv2.float()).all())
    ref, lim = R.gate_grad(R.attn_delta(P.heads(P.q, Nq), P.heads(P2.k, Nk2), P.heads(P2.v, Nk2), P.heads(P.dy.reshape(B * Nq, P.C), Nq), P.scale))
    near("attention gate gradient against float64", gg, ref, lim + 1e-30, "checkpointed" if checkpointed else "plain")


def test_checkpoint_of_a_segment_without_gradients_records_nothing(ops):
    x, gamma, beta, w, r, _ = R.segment_operands()
    xd, gd, bd, wd, rd = dv(x), gamma.to(DEV), beta.to(DEV), dv(w), dv(r)
    tape = Tape()
    with tape.recording():
        y = tape.checkpoint(lambda: ops.geglu(ops.gemm(ops.layernorm(xd, gd, bd, 1e-5), wd, residual=rd)))
    assert not tape.nodes and not tape.needs(y) and not tape.keep
    bits("checkpoint forward", cpu(y), cpu(ops.geglu(ops.gemm(ops.layernorm(xd, gd, bd, 1e-5), wd, residual=rd))), "nothing recorded")


# ====================================================================================================== D. refusals
def test_refusals(ops, monkeypatch):
    """everything the tape cannot differentiate raises before the operator is launched, and records nothing"""
    launches = [Spy(monkeypatch, ops.lib, n) for n in ("ae_gemm_bf16", "ae_ln_gemm_bf16", "ae_conv3x3_bf16", "ae_attn_fwd_bf16")]
    g = R.gen(2900)
    a, w, x = dv(R.rnd(g, 7, 40)), dv(R.rnd(g, 72, 40)), dv(R.rnd(g, 2 * 3 * 5, 8))
    wp = ops.pack_conv3x3(dv(R.rnd(g, 8, 8, 3, 3), F32))
    bias, addvec = dv(torch.randn(72, generator=g), F32), dv(torch.randn(1, 72, generator=g), F32)
    cbias, caddvec = dv(torch.randn(8, generator=g), F32), dv(torch.randn(2, 8, generator=g), F32)

    def tape_with(*need):
        t = Tape()
        for n in need:
            t.require(n)
        return t

    def refused(tape, fn, match):
        with pytest.raises(RuntimeError, match=match):
            with tape.recording():
                fn()
        assert not tape.nodes, "a refused call records nothing"
    refused(tape_with(a), lambda: ops.gemm(a, w, epilogue=ops.EPI_GELU), "fused activations")
    refused(tape_with(a), lambda: ops.gemm(a, w, out_f32=True), "fp32 outputs")
    refused(tape_with(addvec), lambda: ops.gemm(a, w, addvec=addvec, rows_per_batch=7), "gemm addvec")
    refused(tape_with(a, addvec), lambda: ops.gemm(a, w, addvec=addvec, rows_per_batch=7), "gemm addvec")
    refused(tape_with(bias), lambda: ops.gemm(a, w, bias), "gemm bias")
    refused(tape_with(x, caddvec), lambda: ops.conv3x3(x, wp, None, 2, 3, 5, addvec=caddvec), "conv3x3 addvec")
    refused(tape_with(caddvec), lambda: ops.conv3x3(x, wp, None, 2, 3, 5, addvec=caddvec), "conv3x3 addvec")
    refused(tape_with(cbias), lambda: ops.conv3x3(x, wp, cbias, 2, 3, 5), "conv3x3 bias")
    t = Tape()
    t.mark_trainable(cbias, "conv.bias")
    refused(t, lambda: ops.conv3x3(x, wp, cbias, 2, 3, 5), "conv3x3 has no bias gradient")
    # a trainable GEMM bias and operands that need no gradient are fine
    t = Tape()
    t.mark_trainable(bias, "b")
    with t.recording():
        ops.gemm(a, w, bias, addvec=addvec, rows_per_batch=7)
        ops.conv3x3(x, wp, cbias, 2, 3, 5, addvec=caddvec)
    assert len(t.nodes) == 1
    assert sum(len(sp.calls) for sp in launches) == 2, "only the two calls that were not refused reached a kernel"
    # attention: decided before any launch
    P = Attn(40, 33, 77, False, 2901, pad=0)
    mask = torch.ones(ATTN_B, 77, dtype=torch.uint8, device=DEV)
    rel = torch.zeros(1, dtype=F32, device=DEV)
    gate = torch.ones(ATTN_B, dtype=F32, device=DEV)
    seg2 = (P.k, P.v, 77, P.ks, P.ks, gate)
    refused(tape_with(P.q), lambda: P.forward(ops, key_mask=mask), "masked / biased")
    refused(tape_with(P.q), lambda: P.forward(ops, rel_h=rel, rel_w=rel, kH=7, kW=11), "masked / biased")
    refused(tape_with(P.q), lambda: P.forward(ops, seg2=seg2, out_scale=gate), "masked / biased")
    refused(tape_with(P.q), lambda: P.forward(ops, accumulate=True, out_scale=gate), "accumulate=True needs")
    assert sum(len(sp.calls) for sp in launches) == 2, "refused before any launch"
    # a gradient for a partial view
    t = tape_with(a)
    with pytest.raises(RuntimeError, match="partial view"):
        t.accumulate(a[:, :8], dv(R.rnd(g, 7, 8)))
    assert t.grad(a[:3]) is None
