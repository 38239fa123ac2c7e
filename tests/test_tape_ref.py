"""CPU checks of tests/tape_ref.py, the references and bounds that tests/test_hip_tape_adjoints.py holds the training tape to.

  * every reference equals torch.autograd of the float64 forward (to float64 rounding);
  * a bf16-storage emulation of every route — float64 arithmetic, built the way anyedit_amd/autodiff.py builds it (transposed weight
    slices, rotated weight, zero-insert and crop, conv at 2H x 2W then 2x2 sums, zero-padded transposes), rounded to bf16 / fp32 exactly
    where the tape stores — stays at or below 1.0 of the bound on every case of the list: the bounds are not too tight for a correct
    implementation."""
import pytest
import torch
import torch.nn.functional as F

import norm_ref
import small_ref
import tape_ref as R

F32, F64 = torch.float32, torch.float64


def ids(c):
    return "-".join(f"{k}={v}" for k, v in c.items() if k != "seed")


def cases(name):
    return pytest.mark.parametrize("c", R.CASES[name], ids=ids)


def ratio(got, ref, bnd):
    return float(((got.to(F64) - ref).abs() / bnd).max())


def same(got, ref, what):
    """two float64 evaluations of one expression: equal up to the order of the sums"""
    tol = 1e-12 * (1.0 + float(ref.abs().max()))
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= tol, what


def f32(t):
    return t.to(F32).to(F64)


# =================================================================================================== GEMM
@cases("gemm_dx")
def test_gemm_data_gradient(c):
    a, w, dy = R.gemm_operands(c)
    ref, ap = R.gemm_dx(dy, w)
    ar = a.clone().requires_grad_(True)
    (ar @ w.t()).backward(dy)
    same(ref, ar.grad, "dX against autograd")
    wt = w.t().contiguous()
    assert ratio(R.q(dy @ wt.t()), ref, R.launch_bound(ref, ap)) <= 1.0


@cases("gemm_split")
def test_gemm_two_source_split(c):
    K1, K2 = c["K1"], c["K2"]
    a12, w, dy = R.gemm_operands(c, K=K1 + K2)
    ref, ap = R.gemm_dx(dy, w)
    a1, a2 = a12[:, :K1].clone().requires_grad_(True), a12[:, K1:].clone().requires_grad_(True)
    (torch.cat([a1, a2], 1) @ w.t()).backward(dy)
    same(ref[:, :K1], a1.grad, "dA against autograd")
    same(ref[:, K1:], a2.grad, "dA2 against autograd")
    wt = w.t().contiguous()
    bnd = R.launch_bound(ref, ap)
    assert ratio(R.q(dy @ wt[:K1].t()), ref[:, :K1], bnd[:, :K1]) <= 1.0
    assert ratio(R.q(dy @ wt[K1:].t()), ref[:, K1:], bnd[:, K1:]) <= 1.0


@cases("gemm_fanout")
@pytest.mark.parametrize("fused", [True, False])
def test_gemm_fanout(c, fused):
    g = R.gen(c["seed"])
    M, N, K = c["M"], c["N"], c["K"]
    a = R.rnd(g, M, K).requires_grad_(True)
    ws = [R.rnd(g, N, K, scale=K ** -0.5) for _ in range(3)]
    dys = [R.rnd(g, M, N) for _ in range(3)]
    pairs = [R.gemm_dx(dy, w) for dy, w in zip(dys, ws)]
    total, bnd = R.fanout_bounds([p[0] for p in pairs], [p[1] for p in pairs], fused)
    sum((a @ w.t() * dy).sum() for w, dy in zip(ws, dys)).backward()
    same(total, a.grad, "fan-out sum against autograd")
    g3 = R.q(pairs[2][0])
    g2 = R.q(g3 + R.q(pairs[1][0]))
    g1 = R.q(g2 + (pairs[0][0] if fused else R.q(pairs[0][0])))
    assert ratio(g1, total, bnd) <= 1.0


@cases("gemm_dw")
def test_gemm_parameter_gradients(c):
    a, w, dy = R.gemm_operands(c)
    M, N, K = c["M"], c["N"], c["K"]
    wr, br = w.clone().requires_grad_(True), torch.zeros(N, dtype=F64, requires_grad=True)
    (a @ wr.t() + br).backward(dy)
    rw, pw = R.gemm_dw(dy, a)
    rb, pb = R.gemm_db(dy)
    same(rw, wr.grad, "dW against autograd")
    same(rb, br.grad, "db against autograd")
    Mp = (M + 7) // 8 * 8
    dyt, at = torch.zeros(N, Mp, dtype=F64), torch.zeros(K, Mp, dtype=F64)
    dyt[:, :M], at[:, :M] = dy.t(), a.t()
    assert ratio(f32(dyt @ at.t()), rw, R.launch_bound(rw, pw, f32=True)) <= 1.0
    assert ratio(f32(dy.sum(0)), rb, R.launch_bound(rb, pb, f32=True)) <= 1.0
    # the weight used by two GEMMs: two fp32 launches, one fp32 addition
    g = R.gen(c["seed"] + 50)
    a2, dy2 = R.rnd(g, M, K), R.rnd(g, M, N)
    rw2, pw2 = R.gemm_dw(dy2, a2)
    tot, bnd = R.sum_of_launches([rw, rw2], [pw, pw2])
    assert ratio(f32(f32(rw) + f32(rw2)), tot, bnd) <= 1.0


# =================================================================================================== conv
def rotated(w):
    """Tape.rotated on the packed layout: w'[ci][ky'][kx'][co] = w[co][2-ky'][2-kx'][ci], as a torch conv weight [Cin, Cout, 3, 3]"""
    cout, cin = w.shape[:2]
    cin_pad = (cin + 63) // 64 * 64
    wp = torch.zeros(cout, 3, 3, cin_pad, dtype=F64)
    wp[..., :cin] = w.permute(0, 2, 3, 1)
    return wp.flip(1, 2).permute(3, 1, 2, 0)[:cin].permute(0, 3, 1, 2).contiguous()


def autograd_dx(c, x, w, dy, stride=1, up=False):
    xr = x.clone().requires_grad_(True)
    R.conv_forward(xr, w, c["B"], c["H"], c["W"], stride, up).backward(dy)
    return xr.grad


@cases("conv_s1")
def test_conv_stride1(c):
    x, w, dy = R.conv_operands(c)
    B, H, W = c["B"], c["H"], c["W"]
    ref, ap = R.conv_dx(dy, w, B, H, W)
    same(ref, autograd_dx(c, x, w, dy), "conv dX against autograd")
    got = R.q(R.to_rows(F.conv2d(R.to_nchw(dy, B, H, W), rotated(w), padding=1)))
    assert ratio(got, ref, R.launch_bound(ref, ap)) <= 1.0


@cases("conv_s2")
def test_conv_stride2(c):
    x, w, dy = R.conv_operands(c, stride=2)
    B, H, W = c["B"], c["H"], c["W"]
    Ho, Wo = R.conv_out_hw(H, W, 2)
    ref, ap = R.conv_dx(dy, w, B, H, W, stride=2)
    same(ref, autograd_dx(c, x, w, dy, stride=2), "stride-2 conv dX against autograd")
    z = torch.zeros(B, c["Cout"], 2 * Ho, 2 * Wo, dtype=F64)      # zero-insert: dy at the even positions
    z[:, :, ::2, ::2] = R.to_nchw(dy, B, Ho, Wo)
    full = F.conv2d(z, rotated(w), padding=1)
    got = R.q(R.to_rows(full[:, :, :H, :W]))                       # the crop of an odd map
    assert ratio(got, ref, R.launch_bound(ref, ap)) <= 1.0
    # what the crop drops would be the gradient of a padding position: the forward never reads x there
    assert full.shape[2] - H == H % 2 and full.shape[3] - W == W % 2


@cases("conv_up")
def test_conv_nearest_up(c):
    x, w, dy = R.conv_operands(c, up=True)
    B, H, W = c["B"], c["H"], c["W"]
    ref, bnd = R.conv_up_dx(dy, w, B, H, W)
    same(ref, autograd_dx(c, x, w, dy, up=True), "nearest-up conv dX against autograd")
    v = R.q(F.conv2d(R.to_nchw(dy, B, 2 * H, 2 * W), rotated(w), padding=1))
    got = R.q(R.to_rows(v.reshape(B, -1, H, 2, W, 2).sum((3, 5))))
    assert ratio(got, ref, bnd) <= 1.0


# =================================================================================================== layout adjoints
@cases("concat")
def test_concat(c):
    g = R.gen(c["seed"])
    rows, ca, cb = c["rows"], c["ca"], c["cb"]
    a, b = R.rnd(g, rows, ca).requires_grad_(True), R.rnd(g, rows, cb).requires_grad_(True)
    dy, old = R.rnd(g, rows, ca + cb), R.rnd(g, rows, ca)
    torch.cat([a, b], 1).backward(dy)
    assert torch.equal(a.grad, dy[:, :ca]) and torch.equal(b.grad, dy[:, ca:])
    ref, bnd = R.concat_add(old, dy[:, :ca])
    assert ratio(R.q(ref), ref, bnd) <= 1.0


@cases("rows_to_nchw")
def test_rows_to_nchw(c):
    g = R.gen(c["seed"])
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    x = R.rnd(g, B * H * W, C).requires_grad_(True)
    dy = torch.randn(B, C, H, W, generator=g).to(F64)
    R.to_nchw(x, B, H, W).backward(dy)
    assert torch.equal(R.nchw_adjoint(dy).to(F64), R.q(x.grad))


def test_gate_gradient_is_the_sum_of_delta():
    g = R.gen(7)
    B, H, Nq, Nk, D = 2, 3, 5, 4, 8
    qh, kh, vh, dO = (R.rnd(g, B, H, n, D) for n in (Nq, Nk, Nk, Nq))
    gate = torch.tensor([0.7, 0.3], dtype=F64, requires_grad=True)
    out = gate.view(B, 1, 1, 1) * (torch.softmax(D ** -0.5 * qh @ kh.transpose(-1, -2), -1) @ vh)
    out.backward(dO)
    ref, lim = R.gate_grad(R.attn_delta(qh, kh, vh, dO, D ** -0.5))
    same(ref, gate.grad, "gate gradient against autograd")
    assert bool((lim > 0).all())


# =================================================================================================== a checkpointed segment
def test_segment_adjoint():
    c = R.SEGMENT
    x, gamma, beta, w, r, dy = R.segment_operands()
    eps = c["eps"]
    # at the exact forward values the staged adjoint is the gradient of the float64 forward
    xr, wr, rr = (t.clone().requires_grad_(True) for t in (x, w, r))
    u = F.layer_norm(xr, (c["C"],), gamma.to(F64), beta.to(F64), eps) @ wr.t() + rr
    a, gt = u[:, :c["F"]], u[:, c["F"]:]
    (a * 0.5 * gt * (1.0 + torch.erf(gt / 2 ** 0.5))).backward(dy)
    h64, u64, _ = R.segment_forward(x, gamma, beta, w, r, eps)
    exact = R.segment_adjoint(x, gamma, beta, w, h64, u64, dy, eps)
    for k, t in (("dx", xr), ("dr", rr), ("dw", wr)):
        assert float((exact[k][0] - t.grad).abs().max()) <= 1e-9 * (1.0 + float(t.grad.abs().max())), k
    # bf16 storage: h, u stored; du, dh, dx stored; dW fp32
    h, uu = R.q(h64), R.q(R.q(h64) @ w.t() + r)
    ref = R.segment_adjoint(x, gamma, beta, w, h, uu, dy, eps)
    du = R.q(small_ref.ref_geglu_bwd(uu, dy)[0])
    dw = f32(du.t() @ h)
    dh = R.q(du @ w)
    dx = R.q(norm_ref.backward(x[:, None, :], gamma, beta, dh[:, None, :], 1, eps, 0, False)["dx"][:, 0, :])
    for k, got in (("dx", dx), ("dr", du), ("dw", dw)):
        assert ratio(got, *ref[k]) <= 1.0, k
