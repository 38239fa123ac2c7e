"""tests/small_ref.py without a GPU.

1. The references against what they restate: every sampler reference equals its stand-in bit for bit in fp32; the gate backward / weight
   gradient references and the GEGLU gradient equal float64 autograd of the forward reference to 1e-12.
2. The bounds against wrong kernels: per bound family the correctly rounded reference passes and each of a list of deliberately wrong
   results — made in torch from the reference, at the sizes of the GPU cases — raises BoundFailure.
3. Conditions on the case data that the GPU tests rely on (gate margins, the atol / rtol switch of the adaptive error).
4. The case table names every `extern "C"` launch entry point of the four sources that anyedit_amd/_lib.py binds.
"""
import os
import re

import pytest
import torch

import small_ref as R
from small_ref import SamplerStandIns as SI, BoundFailure

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS = tuple(R.c32(v) for v in (0.94, 0.3410, 0.3976, 0.9149, 0.07))


def fails(fn, *a):
    with pytest.raises(BoundFailure):
        fn(*a)


# ====================================================================================================== 1. references
@pytest.mark.parametrize("branches", [1, 2, 3])
@pytest.mark.parametrize("noise", [False, True])
def test_ddim_references_equal_the_stand_ins(branches, noise):
    g = R.gen(1)
    x, nz = R.randn(g, 3, 4, 5, 7), R.randn(g, 3, 4, 5, 7)
    eps = R.randn(g, branches * 3, 4, 5, 7)
    kw = dict(s0=7.5, s1=1.5, noise=nz if noise else None, temperature=0.8)
    for got, ref in zip(R.ref_ddim_step(x, eps, COEFFS, branches, **kw), SI.ddim_step(x, eps, COEFFS, branches, want_e=True, **kw)):
        R.check_bits(got, ref.contiguous(), "ddim_step")
    if branches < 3:
        R.check_bits(R.ref_ddim_encode_step(x, eps, 1.0123, -0.0456, branches, 7.5), SI.ddim_encode_step(x, eps, 1.0123, -0.0456, branches, 7.5), "encode")


def test_plms_mask_blend_q_sample_references_equal_the_stand_ins():
    g = R.gen(2)
    e = R.randn(g, 3, 4, 5, 7)
    hist = [R.randn(g, 3, 4, 5, 7) for _ in range(4)]
    R.check_bits(R.ref_plms(e, [hist[0]], 0), SI.plms_combine_first(e, hist[0]), "plms first")
    for n in (1, 2, 3, 4):
        R.check_bits(R.ref_plms_combine(e, hist[:n]), SI.plms_combine(e, hist[:n]), f"plms history {n}")
    R.check_bits(R.ref_plms_combine(e, hist), R.ref_plms(e, [hist[3], hist[2], hist[1]], 3), "a history of four uses the newest three")
    img, x0, nz = (R.randn(g, 3, 4, 5, 7) for _ in range(3))
    for shape in ((3, 1, 5, 7), (1, 1, 5, 7), (3, 4, 5, 7)):
        m = torch.rand(*shape, generator=g)
        for order in (False, True):
            R.check_bits(R.ref_mask_blend(img, x0, nz, m, 0.73, 0.68, order), SI.mask_blend(img, x0, nz, m, R.c32(0.73), R.c32(0.68), order), "mask_blend")
    sa, s1 = torch.tensor([0.73, 0.2, 0.99]), torch.tensor([0.68, 0.97, 0.1])
    R.check_bits(R.ref_q_sample(x0, nz, sa, s1), SI.q_sample(x0, nz, sa, s1), "q_sample")


@pytest.mark.parametrize("c", R.CASES["ae_dpm_multistep_f32"][:-1], ids=str)
def test_dpm_multistep_reference_equals_the_stand_in(c):
    x, out, mp, kw = dpm_operands(c)
    m, xn = R.ref_dpm_multistep(x, out, c["branches"], 7.5, 0.61, 0.79, **kw)
    ms, xs = SI.dpm_multistep(x, out, c["branches"], R.c32(7.5), R.c32(0.61), R.c32(0.79), **{k: (tuple(R.c32(u) for u in v) if k == "update" and v else v)
                                                                                                  for k, v in kw.items()})
    R.check_bits(m, ms.contiguous(), "m")
    assert (xn is None) == (xs is None)
    if xn is not None:
        R.check_bits(xn, xs.contiguous(), "x_next")


def dpm_operands(c):
    g = R.gen(3)
    n = c["n"]
    x, out, mp = R.randn(g, n), R.randn(g, c["branches"] * n), R.randn(g, n)
    upd = {"none": None, "first": (1.07, 0.31, 0.0, 0.0), "second": (1.07, 0.31, 0.155, 1.9)}[c["update"]]
    return x, out, mp, dict(predict_x0=bool(c["predict_x0"]), v_param=bool(c["v_param"]), m_prev=mp if c["update"] == "second" else None, update=upd)


def test_lincomb_and_adaptive_error_references_agree_with_the_stand_ins():
    g = R.gen(4)
    ts = [(R.randn(g, 4099), c) for c in (1.3, -0.4, 0.07, 2.5)]
    for k in (1, 2, 3, 4):
        ref, bnd = R.ref_lincomb(ts[:k])
        assert R.check_elements(SI.lincomb(ts[:k]), ref, bnd, "lincomb") <= 1.0
    for c in R.CASES["ae_dpm_adaptive_err_f32"]:
        xl, xh, xp, atol, rtol = R.adaptive_case(c)
        ref, bnd = R.ref_dpm_adaptive_err(xl, xh, xp, atol, rtol)
        assert R.check_elements(SI.dpm_adaptive_err(xl, xh, xp, atol, rtol), ref, bnd, "adaptive") <= 1.0


@pytest.mark.parametrize("c", R.CASES["ae_task_gate_bwd"], ids=str)
def test_gate_gradients_equal_autograd_of_the_forward(c):
    te, code, Wg, bg = R.gate_case(c)
    f = R.ref_task_gate(te, code, Wg, bg)
    dgate = R.randn(R.gen(5), code.numel()).to(F64)
    te_rows = te.to(F64)[code.clamp(0, te.shape[0] - 1)].clone().requires_grad_(True)
    W, b = Wg.to(F64).clone().requires_grad_(True), bg.to(F64).clone().requires_grad_(True)
    gate = torch.softmax(te_rows @ W.t() + b, -1)[torch.arange(code.numel()), f["top1"]]      # top1 held constant
    gate.backward(dgate)
    dte, _ = R.ref_task_gate_bwd(f["probs"], f["top1"], dgate, Wg)
    (dW, _), (db, _) = R.ref_task_gate_wgrad(f["probs"], f["top1"], dgate, te, code)
    for got, ref in ((dte, te_rows.grad), (dW, W.grad), (db, b.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_geglu_gradient_equals_autograd():
    g = R.gen(6)
    h = (torch.rand(37, 48, generator=g, dtype=F64) * 12 - 6).requires_grad_(True)
    dy = torch.randn(37, 24, generator=g, dtype=F64)
    y = h[:, :24] * torch.nn.functional.gelu(h[:, 24:])
    y.backward(dy)
    ref, _ = R.ref_geglu_bwd(h.detach(), dy)
    fwd, _ = R.ref_geglu(h.detach())
    assert float((fwd - y.detach()).abs().max()) <= 1e-12 and float((ref - h.grad).abs().max()) <= 1e-12


def test_adamw_reference_is_torch_adamw():
    g = R.gen(7)
    p0 = R.randn(g, 1025)
    pt = p0.to(F64).clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    p, m, v = p0, torch.zeros(1025), torch.zeros(1025)
    for step in (1, 2, 3):
        gr = R.randn(g, 1025)
        pt.grad = gr.to(F64)
        opt.step()
        p, m, v = R.ref_adamw(p, gr, m, v, step, 1e-3)
    assert float((p - pt.detach()).abs().max()) <= 1e-6 * 1e-3     # the fp32 hyper-parameters of the C ABI against python doubles


# ====================================================================================================== 2. mutants
def test_family_a_bit_exact_rejects_wrong_indices_orders_and_skipped_passes():
    g = R.gen(10)
    n = R.GRID_WRAP
    x, nz = R.randn(g, n), R.randn(g, n)
    eps = R.randn(g, 2 * n)
    xp, p0, e = R.ref_ddim_step(x, eps, COEFFS, 2, s0=7.5, noise=nz)
    assert R.check_bits(xp.clone(), xp, "x_prev") == 0.0
    # the grid-stride second pass skipped: elements >= 4096 * 256 left at the sentinel
    skipped = xp.clone()
    skipped.view(torch.int32)[4096 * 256:] = 0x7FA5A5A5
    fails(R.check_bits, skipped, xp, "second pass")
    # cond and uncond swapped
    fails(R.check_bits, R.ref_ddim_step(x, torch.cat([eps[n:], eps[:n]]), COEFFS, 2, s0=7.5, noise=nz)[0], xp, "swap")
    # one element off by one ulp, and -0 for +0
    ulp = xp.clone()
    ulp.view(torch.int32)[n - 1] += 1
    fails(R.check_bits, ulp, xp, "ulp")
    fails(R.check_bits, -torch.zeros(4), torch.zeros(4), "sign of zero")
    # 1 - mask swapped; the other order
    img, x0, no = (R.randn(g, 3, 4, 5, 7) for _ in range(3))
    m = torch.rand(3, 1, 5, 7, generator=g)
    ref = R.ref_mask_blend(img, x0, no, m, 0.73, 0.68)
    fails(R.check_bits, R.ref_mask_blend(img, x0, no, 1.0 - m, 0.73, 0.68), ref, "1 - mask")
    fails(R.check_bits, R.ref_mask_blend(img, x0, no, m, 0.73, 0.68, True), ref, "order")
    # the mask plane of the neighbouring sample
    fails(R.check_bits, R.ref_mask_blend(img, x0, no, m.roll(1, 0), 0.73, 0.68), ref, "mask sample")
    # q_sample: the coefficient of the neighbouring sample (i / per_sample off by one at a sample's first element)
    sa, s1 = torch.tensor([0.73, 0.2, 0.99]), torch.tensor([0.68, 0.97, 0.1])
    a, b = R.randn(g, 3, 257), R.randn(g, 3, 257)
    ref = R.ref_q_sample(a, b, sa, s1)
    bad = ref.clone()
    bad[1, 0] = sa[0] * a[1, 0] + s1[0] * b[1, 0]
    fails(R.check_bits, bad, ref, "q_sample index")
    # PLMS order shifted by one, and a history of four that uses the oldest three
    e_t = R.randn(g, 420)
    hist = [R.randn(g, 420) for _ in range(4)]
    for k in (1, 2, 3):
        fails(R.check_bits, R.ref_plms(e_t, hist[:3][::-1], k - 1), R.ref_plms(e_t, hist[:3][::-1], k), "plms order")
    fails(R.check_bits, R.ref_plms(e_t, hist[:3][::-1], 3), R.ref_plms_combine(e_t, hist), "plms oldest three")
    # data movement: the last vector of a row dropped (concat), padding not zero (transpose), a double rounding that is none (patchify)
    ra, rb = R.randn(g, 5, 8, dtype=BF), R.randn(g, 5, 16, dtype=BF)
    ref = torch.cat([ra, rb], 1)
    bad = ref.clone()
    bad[4, 16:] = 0
    fails(R.check_bits, bad, ref, "last vector")
    t = R.ref_transpose(R.randn(g, 2, 20, 63), 24, BF)
    assert bool((t[:, :, 20:] == 0).all())
    bad = t.clone()
    bad.view(torch.int16)[1, 62, 23] = -32768
    fails(R.check_bits, bad, t, "padding")
    xx = R.randn(g, 2, 3, 28, 42)
    fails(R.check_bits, R.ref_patchify(xx.transpose(2, 3).contiguous(), 14), R.ref_patchify(xx, 14), "patch order")


def test_family_b_rejects_ignored_accumulate_double_rounding_and_dropped_vectors():
    g = R.gen(11)
    dy, oa, ob = R.randn(g, 5, 24, dtype=BF), R.randn(g, 5, 8, dtype=BF), R.randn(g, 5, 16, dtype=BF)
    (ra, ba), (rb, bb) = R.ref_split(dy, 8, oa, ob)
    assert R.check_elements(ra.to(BF), ra, ba, "a") <= 1.0 and R.check_elements(rb.to(BF), rb, bb, "b") <= 1.0
    fails(R.check_elements, dy[:, 8:], rb, bb, "accumulate ignored")
    fails(R.check_elements, (dy[:, :8].float() + ob[:, :8].float()).to(BF), ra, ba, "the other target's old value")
    # sumpool: pairwise sums rounded to bf16 before the last add (a result rounded twice)
    x = R.randn(g, 2 * 6 * 10, 8, dtype=BF)
    ref, bnd = R.ref_sumpool2x2(x, 2, 3, 5)
    assert R.check_elements(ref.to(BF), ref, bnd, "sumpool") <= 1.0
    t = x.float().reshape(2, 3, 2, 5, 2, 8)
    twice = ((t[:, :, 0, :, 0] + t[:, :, 0, :, 1]).to(BF).float() + (t[:, :, 1, :, 0] + t[:, :, 1, :, 1]).to(BF).float()).to(BF).reshape(-1, 8)
    fails(R.check_elements, twice, ref, bnd, "rounded twice")
    fails(R.check_elements, R.ref_mean2x2(x, 2, 6, 10)[0].to(BF), ref, bnd, "mean for sum")
    # the 2x2 mean of odd sizes floors: windows taken from the un-cropped row pitch are wrong
    xm = R.randn(g, 2 * 5 * 7, 16, dtype=BF)
    ref, bnd = R.ref_mean2x2(xm, 2, 5, 7)
    assert ref.shape == (2 * 2 * 3, 16) and R.check_elements(ref.to(BF), ref, bnd, "mean") <= 1.0
    fails(R.check_elements, R.ref_mean2x2(xm.reshape(2, 5, 7, 16)[:, :, 1:].reshape(-1, 16), 2, 5, 6)[0].to(BF), ref, bnd, "column offset")
    # add / axpy: the last vector dropped at n = 2056, alpha ignored, a sample index off by one in add_bcast and scale_shift
    a, b = R.randn(g, 2056, dtype=BF), R.randn(g, 2056, dtype=BF)
    for alpha in (0.0, 1.0, -0.5, 2.75):
        ref, bnd = R.ref_axpy(a, b, alpha)
        assert R.check_elements(ref.to(BF), ref, bnd, "axpy") <= 1.0
        bad = ref.to(BF).clone()
        bad[2048:] = 0
        fails(R.check_elements, bad, ref, bnd, "last vector")
        if alpha != 1.0:
            fails(R.check_elements, (a.float() + b.float()).to(BF), ref, bnd, "alpha ignored")
    xb, p = R.randn(g, 3, 320, dtype=BF), R.randn(g, 320, dtype=BF)
    ref, bnd = R.ref_add_bcast(xb, p)
    assert R.check_elements(ref.to(BF), ref, bnd, "add_bcast") <= 1.0
    fails(R.check_elements, (xb.float() + p.float().roll(8)).to(BF), ref, bnd, "period offset")
    xs, emb = R.randn(g, 15, 16, dtype=BF), R.randn(g, 3, 32)
    ref, bnd = R.ref_scale_shift(xs, emb, 3, 5, False)
    assert R.check_elements(ref.to(BF), ref, bnd, "scale_shift") <= 1.0
    fails(R.check_elements, R.ref_scale_shift(xs, emb.roll(1, 0), 3, 5, False)[0].to(BF), ref, bnd, "neighbouring sample")
    fails(R.check_elements, R.ref_scale_shift(xs, torch.cat([emb[:, 16:], emb[:, :16]], 1), 3, 5, False)[0].to(BF), ref, bnd, "scale and shift swapped")
    # mse_grad (fp32): the loss scale dropped, a result rounded through bf16
    pr, tg = R.randn(g, 4100), R.randn(g, 4100)
    ref, bnd = R.ref_mse_grad(pr, tg, 128.0)
    assert R.check_elements(ref.float(), ref, bnd, "mse_grad") <= 1.0
    fails(R.check_elements, R.ref_mse_grad(pr, tg, 1.0)[0].float(), ref, bnd, "loss scale")
    fails(R.check_elements, ref.to(BF).float(), ref, bnd, "rounded through bf16")


def test_family_c_rejects_a_missing_clamp_a_wrong_function_and_double_rounding():
    g = R.gen(12)
    lv = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0])[torch.randint(0, 5, (3, 4, 35), generator=g)]
    mom = torch.cat([R.randn(g, 3, 4, 35), lv], 1)
    nz = R.randn(g, 3, 4, 35)
    f = R.ref_gaussian(mom, nz)
    for k in ("z", "std"):
        assert R.check_elements(f[k].float(), f[k], R.bound_c32(f[k]), k) <= 1.0
    # one end of the clamp missing.  exp(-15) = 3e-7 is below a (|ref| + 1), so the lower end shows in the logvar output (moved: bit-exact) alone
    for lo, hi in ((-1e9, 20.0), (-30.0, 1e9)):
        fails(R.check_bits, lv.clamp(lo, hi), f["logvar"].float(), "logvar not clamped")
    std = torch.exp(0.5 * lv.to(F64).clamp(-30.0, 1e9))
    fails(R.check_elements, std.float(), f["std"], R.bound_c32(f["std"]), "clamp")
    fails(R.check_elements, (mom[:, :4].to(F64) + std * nz.to(F64)).float(), f["z"], R.bound_c32(f["z"]), "clamp in z")
    fails(R.check_bits, lv, f["logvar"].float(), "logvar not clamped")
    fails(R.check_elements, f["std"].to(BF).float(), f["std"], R.bound_c32(f["std"]), "rounded through bf16")
    fails(R.check_elements, R.ref_gaussian(mom, nz.roll(1, 0))["z"].float(), f["z"], R.bound_c32(f["z"]), "noise of the neighbouring sample")
    # SiLU in +-100, against sigmoid alone, tanh-GELU for erf-GELU, two bf16 ulps
    x = (torch.rand(257, generator=g) * 200 - 100)
    ref, bnd = R.ref_silu(x)
    assert R.check_elements(ref.to(BF), ref, bnd, "silu") <= 1.0
    fails(R.check_elements, torch.nn.functional.gelu(x.to(F64)).to(BF), ref, bnd, "gelu for silu")
    i = int((ref.abs() * R.BF_EPS / bnd).argmax())
    bad = ref.to(BF).clone()
    bad.view(torch.int16)[i] += 2
    fails(R.check_elements, bad, ref, bnd, "two ulps")
    h = (torch.rand(37, 48, generator=g) * 12 - 6).to(BF)
    dy = R.randn(g, 37, 24, dtype=BF)
    ref, bnd = R.ref_geglu(h)
    assert R.check_elements(ref.to(BF), ref, bnd, "geglu") <= 1.0
    a64, g64 = h.to(F64)[:, :24], h.to(F64)[:, 24:]
    fails(R.check_elements, (a64 * torch.nn.functional.gelu(g64, approximate="tanh")).to(BF), ref, bnd, "tanh gelu")
    fails(R.check_elements, (g64 * R.gelu64(a64)).to(BF), ref, bnd, "halves swapped")
    ref, bnd = R.ref_geglu_bwd(h, dy)
    assert R.check_elements(ref.to(BF), ref, bnd, "geglu_bwd") <= 1.0
    d64 = dy.to(F64)
    fails(R.check_elements, torch.cat([d64 * R.gelu64(g64), d64 * a64 * 0.5 * (1 + torch.erf(g64 / 2 ** 0.5))], 1).to(BF), ref, bnd, "pdf term dropped")
    # softmax over a strided row: the last column left out of the sum, the scale ignored, the row maximum of the neighbouring row
    S = (torch.rand(3, 257, generator=g) * 160 - 80)
    ref, bnd = R.ref_softmax_rows(S, 0.0442)
    assert R.check_elements(ref.to(BF), ref, bnd, "softmax") <= 1.0
    short = torch.softmax(S.to(F64)[:, :256] * R.c32(0.0442), -1)
    fails(R.check_elements, torch.cat([short, (ref[:, 256:] * short.sum(-1, keepdim=True) / ref[:, :256].sum(-1, keepdim=True))], 1).to(BF), ref, bnd, "last column")
    fails(R.check_elements, R.ref_softmax_rows(S, 1.0)[0].to(BF), ref, bnd, "scale")
    # the timestep embedding's tolerance: sin for cos
    t = torch.tensor([0.0, 999.5, 21.0])
    ref = R.ref_timestep_embedding(t, 7)
    assert ref.shape == (3, 7) and bool((ref[:, 6] == 0).all())
    assert R.check_elements(ref.float(), ref, R.TIMESTEP_TOL, "embedding") <= 1.0
    fails(R.check_elements, torch.cat([ref[:, 3:6], ref[:, :3], ref[:, 6:]], 1).float(), ref, R.TIMESTEP_TOL, "sin | cos")


def test_family_d_rejects_dropped_terms_skipped_passes_and_wrong_samples():
    g = R.gen(13)
    # mse: the second grid pass skipped (elements past 1024 * 256 not summed), the mean over the wrong count
    a, b = R.randn(g, R.MSE_WRAP), R.randn(g, R.MSE_WRAP)
    ref, bnd = R.ref_mse(a, b)
    assert R.check_elements(ref.float(), ref, bnd, "mse") <= 1.0
    d = (a - b).to(F64)
    fails(R.check_elements, ((d[:1024 * 256] ** 2).sum() / d.numel()).float(), ref, bnd, "second pass")
    fails(R.check_elements, ((d ** 2).sum() / (1024 * 256)).float(), ref, bnd, "mean over one pass's count")
    fails(R.check_elements, ref.to(BF).float(), ref, bnd, "rounded through bf16")
    # rowsum over rows of 1029 (rows start on different alignments): the last vector / the last element dropped, the neighbouring row
    x = R.randn(g, 3, 1029)
    ref, bnd = R.ref_rowsum(x)
    assert R.check_elements(x.sum(1), ref, bnd, "rowsum") <= 1.0
    fails(R.check_elements, x[:, :1025].to(F64).sum(1).float(), ref, bnd, "last vector")
    fails(R.check_elements, x[:, :1028].to(F64).sum(1).float(), ref, bnd, "last element")
    fails(R.check_elements, ref.roll(1).float(), ref, bnd, "row index")
    xc = R.randn(g, 7, 257, dtype=BF)
    ref, bnd = R.ref_colsum(xc)
    assert R.check_elements(ref.float(), ref, bnd, "colsum") <= 1.0
    fails(R.check_elements, xc[:6].to(F64).sum(0).float(), ref, bnd, "last row")
    bad = ref.float().clone()
    bad[256] = 0
    fails(R.check_elements, bad, ref, bnd, "column 256")
    # lincomb: a coefficient of the neighbouring term, the scalar tail left out
    ts = [(R.randn(g, 4099), c) for c in (1.3, -0.4, 0.07, 2.5)]
    ref, bnd = R.ref_lincomb(ts)
    assert R.check_elements(ref.float(), ref, bnd, "lincomb") <= 1.0
    fails(R.check_elements, R.ref_lincomb([(ts[0][0], 1.3), (ts[1][0], -0.4), (ts[2][0], 2.5), (ts[3][0], 0.07)])[0].float(), ref, bnd, "coefficients")
    bad = ref.float().clone()
    bad[4096:] = 0
    fails(R.check_elements, bad, ref, bnd, "tail")
    # adaptive error: the sample index off by one, atol ignored, the mean over the padded count
    for c in R.CASES["ae_dpm_adaptive_err_f32"]:
        xl, xh, xp, atol, rtol = R.adaptive_case(c)
        ref, bnd = R.ref_dpm_adaptive_err(xl, xh, xp, atol, rtol)
        assert R.check_elements(ref.float(), ref, bnd, "adaptive") <= 1.0
        fails(R.check_elements, R.ref_dpm_adaptive_err(xl, xh.roll(1, 0), xp, atol, rtol)[0].float(), ref, bnd, "sample index")
        fails(R.check_elements, R.ref_dpm_adaptive_err(xl, xh, xl, atol, rtol)[0].float(), ref, bnd, "x_prev ignored")
        if c["n"] > 1:
            fails(R.check_elements, R.ref_dpm_adaptive_err(xl, xh, xp, 1e-9, rtol)[0].float(), ref, bnd, "atol ignored")
    # scatter-add: the prefilled rows ignored, only the first row of a code added, an untouched row changed
    src, dst = R.randn(g, 6, 255), R.randn(g, 7, 255)
    code = torch.tensor([2, 0, 2, 5, 2, 0])
    ref, bnd = R.ref_scatter_add_rows(src, code, dst)
    assert R.check_elements(ref.float(), ref, bnd, "scatter") <= 1.0
    fails(R.check_elements, R.ref_scatter_add_rows(src, code, torch.zeros(7, 255))[0].float(), ref, bnd, "accumulate ignored")
    last = dst.to(F64).clone()
    last[code] = dst.to(F64)[code] + src.to(F64)            # index_put without accumulate: one sample per row survives
    fails(R.check_elements, last.float(), ref, bnd, "repeated codes")
    # SAM relative-position terms: the table row of the neighbouring query row / column, the last k left out
    q, Rh, Rw = R.randn(g, 2, 20, 3, 48, dtype=BF), R.randn(g, 4, 7, 48), R.randn(g, 5, 17, 48)
    (rh, bh), (rw, bw) = R.ref_relpos(q, Rh, Rw, 4, 5)
    assert R.check_elements(rh.float(), rh, bh, "rel_h") <= 1.0 and R.check_elements(rw.float(), rw, bw, "rel_w") <= 1.0
    (xh, _), (xw, _) = R.ref_relpos(q, Rh.roll(1, 0), Rw.roll(1, 0), 4, 5)
    fails(R.check_elements, xh.float(), rh, bh, "row")
    fails(R.check_elements, xw.float(), rw, bw, "column")
    fails(R.check_elements, R.ref_relpos(q, Rw[:4, :7], Rh.repeat(2, 3, 1)[:5, :17], 4, 5)[0][0].float(), rh, bh, "tables swapped")
    fails(R.check_elements, R.ref_relpos(q.roll(1, 2), Rh, Rw, 4, 5)[0][0].float(), rh, bh, "head")


def test_gate_bounds_reject_a_tie_to_the_higher_index_and_wrong_samples():
    tie = [c for c in R.CASES["ae_task_gate"] if c.get("tie")][0]
    te, code, Wg, bg = R.gate_case(tie)
    f = R.ref_task_gate(te, code, Wg, bg)
    lo, hi = tie["tie"]
    assert int(f["top1"][0]) == lo and float(f["logits"][0, lo]) == float(f["logits"][0, hi])
    assert R.check_elements(f["probs"].float(), f["probs"], f["bnd"], "probs") <= 1.0
    higher = f["top1"].clone()
    higher[0] = hi
    fails(R.check_bits, higher, f["top1"], "tie to the higher index")
    # the code clamp missing (wrapped instead), bg ignored, the embedding of the neighbouring sample
    n_tasks = te.shape[0]
    fails(R.check_elements, R.ref_task_gate(te, code % n_tasks, Wg, bg)["probs"].float(), f["probs"], f["bnd"], "clamp")
    fails(R.check_elements, R.ref_task_gate(te, code, Wg, None)["probs"].float(), f["probs"], f["bnd"], "bias")
    fails(R.check_elements, R.ref_task_gate(te, code.roll(1), Wg, bg)["probs"].float(), f["probs"], f["bnd"], "sample")
    for c in R.CASES["ae_task_gate_bwd"]:
        te, code, Wg, bg = R.gate_case(c)
        f = R.ref_task_gate(te, code, Wg, bg)
        p32, dg = f["probs"].float(), R.randn(R.gen(5), code.numel())
        ref, bnd = R.ref_task_gate_bwd(p32, f["top1"], dg, Wg)
        assert R.check_elements(ref.float(), ref, bnd, "dte") <= 1.0
        fails(R.check_elements, R.ref_task_gate_bwd(p32, f["top1"].roll(1), dg, Wg)[0].float(), ref, bnd, "top1 of the neighbour")
        fails(R.check_elements, R.ref_task_gate_bwd(p32, f["top1"], dg.roll(1), Wg)[0].float(), ref, bnd, "dgate of the neighbour")
        (dW, bW), (db, bb) = R.ref_task_gate_wgrad(p32, f["top1"], dg, te, code)
        assert R.check_elements(dW.float(), dW, bW, "dWg") <= 1.0 and R.check_elements(db.float(), db, bb, "dbg") <= 1.0
        (xW, _), (xb, _) = R.ref_task_gate_wgrad(p32[:-1], f["top1"][:-1], dg[:-1], te, code[:-1])
        fails(R.check_elements, xW.float(), dW, bW, "last sample dropped")
        fails(R.check_elements, xb.float(), db, bb, "last sample dropped")
        fails(R.check_elements, R.ref_task_gate_wgrad(p32, f["top1"], dg, te, code.roll(1))[0][0].float(), dW, bW, "repeated codes mixed up")


def test_family_e_rejects_the_neighbours_expert_and_double_rounding():
    c = R.CASES["ae_expert_kv_fwd"][1]
    g = R.gen(c["seed"])
    B, T, N, Dc, E = (c[k] for k in ("B", "T", "N", "Dc", "E"))
    x, dy, W = R.randn(g, B * T, Dc, dtype=BF), R.randn(g, B * T, N, dtype=BF), R.randn(g, E, N, Dc, scale=Dc ** -0.5)
    ex = R.expert_ids(c)
    assert len(set(ex.tolist())) > 1
    ref, bnd = R.ref_expert_fwd(x, W, ex, T)
    assert R.check_elements(ref.to(BF), ref, bnd, "fwd") <= 1.0
    fails(R.check_elements, R.ref_expert_fwd(x, W, ex.roll(1), T)[0].to(BF), ref, bnd, "expert of the neighbouring sample")
    fails(R.check_elements, R.ref_expert_fwd(x[:, :256], W[:, :, :256], ex, T)[0].to(BF), ref, bnd, "k past 256 dropped")
    halves = R.ref_expert_fwd(x[:, :128], W[:, :, :128], ex, T)[0].to(BF).float() + R.ref_expert_fwd(x[:, 128:], W[:, :, 128:], ex, T)[0].to(BF).float()
    fails(R.check_elements, halves.to(BF), ref, bnd, "rounded twice")
    fails(R.check_elements, torch.einsum("btk,bnk->btn", x.to(F64).reshape(B, T, Dc), W.to(F64)[ex]).reshape(B * T, N).to(BF)[:, :0], ref, bnd, "shape")
    ref, bnd = R.ref_expert_dgrad(dy, W, ex, T)
    assert R.check_elements(ref.to(BF), ref, bnd, "dgrad") <= 1.0
    fails(R.check_elements, R.ref_expert_dgrad(dy, W, ex.roll(1), T)[0].to(BF), ref, bnd, "expert of the neighbouring sample")
    fails(R.check_elements, R.ref_expert_dgrad(dy[:, :16], W[:, :16], ex, T)[0].to(BF), ref, bnd, "second row group dropped")
    ref, bnd = R.ref_expert_wgrad(dy, x, ex, T, E)
    assert R.check_elements(ref.float(), ref, bnd, "wgrad") <= 1.0
    fails(R.check_elements, R.ref_expert_wgrad(dy, x, ex.roll(1), T, E)[0].float(), ref, bnd, "expert of the neighbouring sample")
    fails(R.check_elements, R.ref_expert_wgrad(dy.reshape(B, T, N)[:, :T - 1].reshape(-1, N), x.reshape(B, T, Dc)[:, :T - 1].reshape(-1, Dc), ex, T - 1, E)[0].float(),
          ref, bnd, "last token dropped")
    one = torch.full((B,), E - 1)
    ref, bnd = R.ref_expert_wgrad(dy, x, one, T, E)
    assert bool((ref[:E - 1] == 0).all()), "experts without a sample: exact zeros"
    bad = ref.float().clone()
    bad[0, 3, 5] = 1e-30
    fails(R.check_elements, bad, ref, bnd, "not a zero")


def test_family_f_rejects_a_wrong_bias_correction_and_coupled_weight_decay():
    g = R.gen(15)
    p, gr, m, v = R.randn(g, 1025), R.randn(g, 1025), R.randn(g, 1025, scale=0.1), R.randn(g, 1025).abs() * 0.01
    for step in (1, 1000):
        ref, mr, vr = R.ref_adamw(p, gr, m, v, step, 1e-3)
        bnd = R.bound_f(ref, 1e-3)
        assert R.check_elements(ref.float(), ref, bnd, "adamw") <= 1.0
        fails(R.check_elements, R.ref_adamw(p, gr, m, v, step + 1 if step == 1 else step // 2, 1e-3)[0].float(), ref, bnd, "bias correction")
        # lr wd |p| = 1e-5 |p| at the cases' lr = 1e-3 is inside a (|p| + lr): weight decay shows at a learning rate of 0.1
        big = R.ref_adamw(p, gr, m, v, step, 0.1)[0]
        fails(R.check_elements, R.ref_adamw(p, gr, m, v, step, 0.1, weight_decay=0.0)[0].float(), big, R.bound_f(big, 0.1), "weight decay")
        fails(R.check_elements, R.ref_adamw(p, gr, m, v, step, 1e-3, grad_scale=1.0 / 128)[0].float(), ref, bnd, "grad scale")
        fails(R.check_elements, ref.to(BF).float(), ref, bnd, "rounded through bf16")


# ====================================================================================================== 3. conditions on the inputs
def test_gate_cases_have_a_clear_winner_and_adaptive_cases_stay_off_the_switch():
    for c in R.CASES["ae_task_gate"] + R.CASES["ae_task_gate_bwd"]:
        te, code, Wg, bg = R.gate_case(c)
        logits, _ = R.gate_forward64(te, code, Wg, bg)
        if logits.shape[1] == 1:
            continue
        top = logits.sort(-1, descending=True).values
        for b in range(logits.shape[0]):
            if c.get("tie") and int(code[b].clamp(0, te.shape[0] - 1)) == 0:
                assert float(top[b, 0]) == float(top[b, 1]) and float(top[b, 1] - top[b, 2]) > 1e-3, c
            else:
                assert float(top[b, 0] - top[b, 1]) > 1e-3, (c, b)
    both = set()
    for c in R.CASES["ae_dpm_adaptive_err_f32"]:
        xl, xh, xp, atol, rtol = R.adaptive_case(c)
        delta, r = R.adaptive_delta(xl, xp, atol, rtol)
        assert float((r / R.c32(atol) - 1.0).abs().min()) > 2.0 ** -20, c
        both |= {bool(v) for v in (r > R.c32(atol)).flatten().tolist()}
    assert both == {True, False}, "both sides of the max in delta"


# ====================================================================================================== 4. the case table is complete
def test_every_launch_entry_point_of_the_four_sources_has_a_case():
    from anyedit_amd import _lib
    exported = set()
    for src in R.SOURCES:
        with open(os.path.join(ROOT, "anyedit_amd", "csrc", src)) as f:
            exported |= set(re.findall(r'extern "C" int (ae_\w+)\(', f.read()))
    bound = {n for n in _lib.SIGNATURES if n in exported} - R.NOT_A_LAUNCH
    assert exported - set(_lib.SIGNATURES) == set(), f"exported but not bound: {sorted(exported - set(_lib.SIGNATURES))}"
    assert bound == set(R.CASES), f"without a case: {sorted(bound - set(R.CASES))}; cases without an entry point: {sorted(set(R.CASES) - bound)}"
    assert all(len(v) > 0 for v in R.CASES.values())
