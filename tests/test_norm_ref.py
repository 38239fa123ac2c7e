"""tests/norm_ref.py without a GPU: its float64 formulas against torch.autograd, and its bounds against five kinds of wrong kernel.

Three cases — a one-launch (two-pass) GroupNorm with a group pack, a three-launch (one-pass) GroupNorm with a ragged last chunk, and the
LayerNorm + window partition with padding on both axes — each as the float64 reference rounded to bf16 (must pass) and corrupted:
  neighbour   one (sample, group) / row normalised with its neighbour's statistics
  twice       the last row of a sample counted twice in the sums (the clamped row of a ragged chunk without its `keep` mask)
  rstd        rstd scaled by 1 + 2^-7
  pad         one element of a padding row not zero
  ulps        one element off by two bf16 ulps
every one of which must fail the element-wise check (and the statistics check where the corruption is in the statistics)."""
import pytest
import torch

import norm_ref as NR

F64, BF = torch.float64, torch.bfloat16
GN_CASES = {
    "slab": dict(B=2, HW=64, C=320, groups=32, act=1, onepass=False, eps=1e-5),
    "three_launch": dict(B=3, HW=257, C=320, groups=32, act=1, onepass=True, eps=1e-5),
}
WIN = dict(B=2, H=20, W=27, C=320, ws=14, eps=1e-6)


def _gn(name):
    c = GN_CASES[name]
    gen = torch.Generator().manual_seed(5)
    x = NR.make_x(gen, c["B"], c["HW"], c["C"], c["groups"])
    gamma, beta = NR.make_affine(gen, c["C"])
    return c, x, gamma, beta, NR.forward(x, gamma, beta, c["groups"], c["eps"], c["act"], c["onepass"])


def _win():
    c = WIN
    gen = torch.Generator().manual_seed(6)
    n = c["B"] * c["H"] * c["W"]
    x = NR.make_x(gen, n, 1, c["C"], 1, const_group=False)
    gamma, beta = NR.make_affine(gen, c["C"])
    return c, x, gamma, beta, NR.forward(x, gamma, beta, 1, c["eps"], 0, False), NR.window_rows(c["B"], c["H"], c["W"], c["ws"])


def _win_out(y, img, C):
    """window rows [rows, C] bf16 of the image rows y [n, 1, C]: padding rows zero"""
    out = torch.zeros(img.numel(), C, dtype=BF)
    out[img >= 0] = y.reshape(-1, C)[img[img >= 0]].to(BF)
    return out


def _win_check(got, f, img, C):
    NR.check_pad_rows(got, img < 0)
    v = img >= 0
    return NR.check_elements(got[v], f["y"].reshape(-1, C)[img[v]], f["bnd"].reshape(-1, C)[img[v]], "output")


def _two_ulps(got, f):
    """got (bf16) with the element whose bound is most nearly the bf16 rounding alone moved by two ulps"""
    i = int((f["y"].abs() * 2.0 ** -8 / f["bnd"]).flatten().argmax())
    bad = got.clone().flatten()
    bad.view(torch.int16)[i] += 2
    return bad.reshape(got.shape)


def test_data_scheme():
    gen = torch.Generator().manual_seed(1)
    x = NR.make_x(gen, 3, 64, 320, 32)
    assert x.dtype == BF
    m, r = NR.statistics(x, 32, 1e-5)
    rho = (m.abs() * r)
    assert int((rho > 300).sum()) == 1, "exactly one constant (sample, group)"
    assert float(rho[rho < 300].max()) > 12 and float(rho.min()) < 0.5, "groups from mean / sigma = 0 to 16"
    g, b = NR.make_affine(gen, 320)
    assert (g == 0).any() and (b == 0).any() and (g < 0).any() and (g > 0).any()


@pytest.mark.parametrize("act", [0, 1])
def test_formulas_agree_with_autograd(act):
    B, HW, C, G, eps = 2, 7, 24, 4, 1e-5
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(B, HW, C, generator=gen, dtype=F64).requires_grad_(True)
    gamma, beta, dy = (torch.randn(s, generator=gen, dtype=F64) for s in ((C,), (C,), (B, HW, C)))
    gamma.requires_grad_(True)
    beta.requires_grad_(True)
    z = torch.nn.functional.group_norm(x.permute(0, 2, 1), G, gamma, beta, eps).permute(0, 2, 1)
    y = torch.nn.functional.silu(z) if act else z
    y.backward(dy)
    with torch.no_grad():
        f = NR.forward(x, gamma, beta, G, eps, act, False)
        b = NR.backward(x, gamma, beta, dy, G, eps, act, False)
        for got, ref in ((f["y"], y), (b["dx"], x.grad)) + (((b["dgamma"], gamma.grad), (b["dbeta"], beta.grad)) if not act else ()):
            assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
        old = torch.randn(B, HW, C, generator=gen, dtype=F64)
        assert torch.allclose(NR.backward(x, gamma, beta, dy, G, eps, act, False, old=old)["dx"], x.grad + old, rtol=0, atol=1e-10)


@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_bounds_pass_the_rounded_reference_and_fail_every_corruption(name):
    c, x, gamma, beta, f = _gn(name)
    G, eps, act, onepass = c["groups"], c["eps"], c["act"], c["onepass"]
    stat = torch.stack([f["mean"], f["rstd"]], -1).float()
    assert NR.check_statistics(stat, f["mean"], f["rstd"], onepass) <= 1.0
    good = f["y"].to(BF)
    assert NR.check_elements(good, f["y"], f["bnd"], "output") <= 1.0

    def wrong(mean, rstd, stats_too):
        got = NR.forward(x, gamma, beta, G, eps, act, onepass, mean=mean, rstd=rstd)["y"].to(BF)
        with pytest.raises(NR.BoundFailure):
            NR.check_elements(got, f["y"], f["bnd"], "output")
        if stats_too:
            with pytest.raises(NR.BoundFailure):
                NR.check_statistics(torch.stack([mean, rstd], -1).float(), f["mean"], f["rstd"], onepass)

    # neighbour: group 3 of sample 0 normalised with group 4's statistics
    m, r = f["mean"].clone(), f["rstd"].clone()
    m[0, 3], r[0, 3] = m[0, 4], r[0, 4]
    wrong(m, r, False)
    # twice: the last row of sample 1 enters the sums a second time
    xg = x.to(F64).reshape(c["B"], c["HW"], G, c["C"] // G)
    n = c["HW"] * (c["C"] // G)
    S, Q = xg.sum((1, 3)), (xg * xg).sum((1, 3))
    S[1] += xg[1, -1].sum(-1)
    Q[1] += (xg[1, -1] ** 2).sum(-1)
    m = S / n
    wrong(m, ((Q / n - m * m).clamp(min=0) + eps).rsqrt(), True)
    # rstd
    wrong(f["mean"], f["rstd"] * (1 + 2.0 ** -7), True)
    # ulps
    with pytest.raises(NR.BoundFailure):
        NR.check_elements(_two_ulps(good, f), f["y"], f["bnd"], "output")


def test_window_partition_bounds_pass_the_rounded_reference_and_fail_every_corruption():
    c, x, gamma, beta, f, img = _win()
    C = c["C"]
    assert int((img < 0).sum()) == c["B"] * (28 * 28 - 20 * 27)
    good = _win_out(f["y"], img, C)
    assert _win_check(good, f, img, C) <= 1.0
    # neighbour: image row 100 normalised with row 101's statistics
    m, r = f["mean"].clone(), f["rstd"].clone()
    m[100], r[100] = m[101], r[101]
    with pytest.raises(NR.BoundFailure):
        _win_check(_win_out(NR.forward(x, gamma, beta, 1, c["eps"], 0, False, mean=m, rstd=r)["y"], img, C), f, img, C)
    # rstd
    with pytest.raises(NR.BoundFailure):
        _win_check(_win_out(NR.forward(x, gamma, beta, 1, c["eps"], 0, False, rstd=f["rstd"] * (1 + 2.0 ** -7))["y"], img, C), f, img, C)
    # pad: the smallest positive bf16 in one padding row (and a negative zero: the kernel stores +0)
    for bits in (1, -32768):
        bad = good.clone()
        bad.view(torch.int16)[int((img < 0).nonzero()[7]), 5] = bits
        with pytest.raises(NR.BoundFailure, match="padding"):
            _win_check(bad, f, img, C)
    # ulps
    v = img >= 0
    bad = good.clone()
    bad[v] = _two_ulps(good[v], dict(y=f["y"].reshape(-1, C)[img[v]], bnd=f["bnd"].reshape(-1, C)[img[v]]))
    with pytest.raises(NR.BoundFailure):
        _win_check(bad, f, img, C)


@pytest.mark.parametrize("name", list(GN_CASES))
@pytest.mark.parametrize("acc", [False, True])
def test_backward_bound_passes_the_rounded_reference_and_fails_two_ulps(name, acc):
    c, x, gamma, beta, _ = _gn(name)
    gen = torch.Generator().manual_seed(8)
    dy = torch.randn(c["B"], c["HW"], c["C"], generator=gen).to(BF)
    old = torch.randn(c["B"], c["HW"], c["C"], generator=gen).to(BF) if acc else None
    b = NR.backward(x, gamma, beta, dy, c["groups"], c["eps"], c["act"], c["onepass"], old=old)
    good = b["dx"].to(BF)
    assert NR.check_elements(good, b["dx"], b["bnd"], "dx") <= 1.0
    # the element most nearly bounded by its rounding alone, moved by two ulps (four under accumulate: two roundings are allowed there)
    i = int((b["dx"].abs() * 2.0 ** -8 / b["bnd"]).flatten().argmax())
    bad = good.clone().flatten()
    bad.view(torch.int16)[i] += 4 if acc else 2
    with pytest.raises(NR.BoundFailure):
        NR.check_elements(bad.reshape(good.shape), b["dx"], b["bnd"], "dx")
    # a sample index error: sample 1's gradient in sample 0's place
    swapped = good.clone()
    swapped[0] = good[1]
    with pytest.raises(NR.BoundFailure):
        NR.check_elements(swapped, b["dx"], b["bnd"], "dx")
