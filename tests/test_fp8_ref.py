"""tests/fp8_ref.py (the float64 model of ae_attn_fwd_fp8 that tests/test_hip_attention_fp8.py holds the kernel to) on the CPU: its e4m3 cast, its
reduction to exact attention, its key permutation, and — for the stored seeds of the GPU cases — the conditions under which model and kernel must
agree (rebase margins, share of uncertain probabilities, the branch a case claims) and that the element bound of the GPU test notices a wrong kernel."""
import numpy as np
import pytest
import torch

import attn_ref as R
import fp8_ref as F

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------------ the cast
def test_every_code_survives_decode_and_cast():
    codes = torch.arange(256, dtype=torch.uint8)
    val = F.e4m3_decode(codes)
    finite = torch.isfinite(val)
    assert int((~finite).sum()) == 2 and not finite[0x7F] and not finite[0xFF]          # e4m3fn: no infinities, one NaN per sign
    assert torch.equal(F.e4m3_bytes(val[finite].to(F32)), codes[finite])
    assert float(val[0x38]) == 1.0 and float(val[0x7E]) == 448.0 and float(val[0x01]) == 2.0 ** -9 and float(val[0x08]) == 2.0 ** -6


def test_midpoints_round_to_even_and_448_stays_finite():
    val = F.e4m3_decode(torch.arange(0x7F, dtype=torch.uint8))          # 0 .. 448, ascending
    mid = ((val[:-1] + val[1:]) / 2).to(F32)                           # exact in fp32
    got = F.e4m3_bytes(mid).to(torch.int64)
    lower = torch.arange(0x7E)
    assert torch.equal(got, lower + (lower & 1)), "a tie must go to the even code"
    for s in (1.0, -1.0):
        assert torch.equal(F.e4m3_bytes(torch.tensor([s * 448.0, s * 449.0, s * 463.9], dtype=F32)).to(torch.int64) & 0x7F, torch.tensor([0x7E] * 3))
    # just beside a midpoint the nearer neighbour wins, and the tie below the smallest subnormal goes to zero
    x = torch.tensor([2.0 ** -10, 2.0 ** -10 * (1 + 2.0 ** -20), 1.0625, 1.0625 * (1 - 2.0 ** -20), 1.0625 * (1 + 2.0 ** -20)], dtype=F32)
    assert F.e4m3_bytes(x).tolist() == [0x00, 0x01, 0x38, 0x38, 0x39]


def test_midpoint_distance():
    x = torch.tensor([1.0625, 1.0, 1.0625 * (1 + 2.0 ** -19), 2.0 ** -10, 0.0, 3 * 2.0 ** -10, 232.0], dtype=F64)
    d, u = F.midpoint_distance(x)
    assert d[0] == 0 and abs(float(d[1]) - 1 / 17) < 1e-15 and abs(float(d[2]) - 2.0 ** -19) < 1e-12 and d[3] == 0 and d[4] == 1 and d[5] == 0
    assert u.tolist() == [0.125, 0.125, 0.125, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 16.0] and d[6] == 0


def test_pow2ceil_and_scales():
    x = np.array([1.0, 1.0000001, 0.75, 3.0, 2.0 ** -100, 1.5 * 2.0 ** -100], dtype=np.float32)
    assert F.pow2ceil(x).tolist() == [1.0, 2.0, 1.0, 4.0, 2.0 ** -100, 2.0 ** -99]
    sc = F.scales(np.array([[4.0, 3.5, 5.0], [0.0, 0.0, 0.0]], dtype=np.float32), 80 ** -0.5)
    # the largest |q| lands in (224, 448] code units, and so does the largest |v|; the largest |k| lands on 448
    assert 224 < 4.0 * sc["qmul"][0] <= 448 and 224 < 5.0 * sc["vmul"][0] <= 448 and abs(3.5 * sc["kmul"][0] - 448) < 1e-3
    # sig qmul kmul = scale log2e: the logits come out in log2 units
    assert abs(float(sc["sig"][0]) * float(sc["qmul"][0]) * float(sc["kmul"][0]) / (80 ** -0.5 * F.LOG2E) - 1) < 1e-6
    assert all(np.isfinite(sc[n][1]) and sc[n][1] > 0 for n in ("qmul", "kmul", "vmul", "sig", "v_pow2")), "an all-zero head keeps finite scales"


def test_mfma64_truncates_products_in_groups_of_eight():
    a, b = torch.zeros(1, 64, dtype=F64), torch.zeros(1, 64, dtype=F64)
    # group 0: E = 4 + 4, quantum 2^-5: 256 stays, 1.125^2 = 1.265625 -> 1.25, its negative -> -1.25 (toward zero), 2^-6 1.125 * 1.125 -> 0
    a[0, :4], b[0, :4] = torch.tensor([16.0, 1.125, -1.125, 2.0 ** -6 * 1.125], dtype=F64), torch.tensor([16.0, 1.125, 1.125, 1.125], dtype=F64)
    # group 1 holds the small product alone: E = -6 + 0, quantum 2^-19: it survives whole
    a[0, 8], b[0, 8] = 2.0 ** -6 * 1.125, 1.125
    got = F.mfma64(a, b, torch.full((1, 1), 3.0, dtype=F64))
    assert float(got) == 3.0 + 256.0 + 1.25 - 1.25 + 2.0 ** -6 * 1.265625
    two = F.mfma64(a, b, torch.zeros(1, 1, dtype=F64), scale=torch.tensor(0.25, dtype=F64))
    assert float(two) == 0.25 * (256.0 + 2.0 ** -6 * 1.265625)
    # one rounding at the end, to fp32
    big = F.mfma64(a, b, torch.full((1, 1), 2.0 ** 20, dtype=F64))
    assert float(big) == float(torch.tensor(2.0 ** 20 + 256.0 + 2.0 ** -6 * 1.265625, dtype=F64).float())


# ------------------------------------------------------------------------------------------------------------ reduction to exact attention
@pytest.mark.parametrize("Nq,Nk,bias", [(37, 130, False), (70, 65, False), (33, 128, True), (129, 192, True), (5, 1, False)])
def test_without_quantisation_the_model_is_exact_attention(Nq, Nk, bias):
    B, H, D = 2, 3, 24
    g = torch.Generator().manual_seed(Nq + Nk)
    q, k, v = (2 * torch.randn(B, H, n, D, generator=g) for n in (Nq, Nk, Nk))
    rel_h = rel_w = None
    if bias:
        rel_h, rel_w = 2 * torch.randn(B * H, Nq, Nk // 64, generator=g), 2 * torch.randn(B * H, Nq, 64, generator=g)
    scale = D ** -0.5
    M = F.model(q, k, v, scale, rel_h, rel_w, quant_operands=False, quant_p=False)
    ref = F.exact_attention(q, k, v, scale, None if rel_h is None else rel_h.reshape(B, H, Nq, -1), None if rel_w is None else rel_w.reshape(B, H, Nq, 64))
    assert float((M.out - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    if not bias:
        ref2 = R.segment(q, k, v, scale)["out"]
        assert float((M.out - ref2).abs().max()) <= 1e-12 * float(ref2.abs().max())
    assert any(bool(r.any()) for r in M.rebased[1:]) or Nk <= 64, "the reduction has to cross a rebase"


def test_model_is_close_to_exact_attention_at_unit_variance():
    x, M = F.case_model("d80")
    e = float((M.out - F.exact_attention(x["q"], x["k"], x["v"], 80 ** -0.5)).norm() / F.exact_attention(x["q"], x["k"], x["v"], 80 ** -0.5).norm())
    assert 2e-2 < e < 8e-2, e


# ------------------------------------------------------------------------------------------------------------ the key permutation
def test_kpos_is_a_bijection_with_the_hand_computed_values():
    assert sorted(F.kpos(k) for k in range(64)) == list(range(64))
    # key 4 = (b2 0, r 0, hi 1) -> 32; key 8 = (r 4) -> 4; key 12 = (r 4, hi 1) -> 36; key 33 = (b2 1, r 1) -> 17; key 63 = (b2 1, r 15, hi 1) -> 63
    for key, pos in ((0, 0), (1, 1), (3, 3), (4, 32), (5, 33), (8, 4), (12, 36), (31, 47), (32, 16), (33, 17), (36, 48), (63, 63)):
        assert F.kpos(key) == pos, (key, F.kpos(key), pos)


def test_workspace_images():
    x, M = F.case_model("img_d40_33x63")
    BH, Nq, Nk, D = 6, 33, 63, 40
    assert M.q8.shape == (BH, Nq, 128) and M.k8.shape == (BH, 64, 128) and M.vt8.shape == (BH, 96, 64)
    assert not M.q8[:, :, D:].any() and not M.k8[:, :, D:].any() and not M.k8[:, Nk:].any()
    assert not M.vt8[:, D + 1:].any() and not M.vt8[:, :, F.kpos(63)].any()
    assert int((M.vt8[:, D] == 0x38).sum()) == BH * Nk
    v8 = F.e4m3_decode(M.vt8[1, :D, F.kpos(12)])
    assert torch.equal(v8, M.V8[1, 12])
    assert float((v8 * float(M.v_pow2[1]) - x["v"].reshape(BH, Nk, D)[1, 12].to(F64)).abs().max()) <= 2.0 ** -4 * float(x["v"].abs().max())


# ------------------------------------------------------------------------------------------------------------ the stored seeds
@pytest.mark.parametrize("name", list(F.CASES))
def test_case_conditions(name):
    c = F.CASES[name]
    _, M = F.case_model(name)
    margin, share, claim = F.conditions(c, M)
    print(f"{name}: margin {margin:.3e} uncertain {M.n_uncertain} of {M.n_prob}")
    assert margin >= 2.0 ** -10, f"{name}: rebase margin {margin:.3e}"
    assert share <= 1e-3, f"{name}: uncertain share {share:.3e}"
    assert claim, f"{name}: does not take the branch it claims ({c.claim})"
    assert bool(torch.isfinite(M.out).all()) and bool((M.allowance >= 0).all()) and bool(torch.isfinite(M.allowance).all())


def test_the_rebase_cases_cover_what_they_name():
    _, M = F.case_model("rebase_none_after_first")
    # rows 32..63: the early key flushes every other probability to zero: the output is that key's quantised value row
    want = (M.v_pow2[:, None] * M.V8[:, 3]).reshape(2, 3, 1, 80).expand(2, 3, 32, 80)
    assert torch.equal(M.out[:, :, 32:64], want)
    _, M = F.case_model("rebase_late")
    assert bool(M.moved[1].all()), "every row moves at the spiked tile"
    _, M = F.case_model("bias_kh1_nq40")
    assert bool((M.moved[0][:, 5::8]).all()) and float(M.margin7[0].min()) >= 2.0 ** -10


# ------------------------------------------------------------------------------------------------------------ the bound notices a wrong kernel
_HEAD_DIMS = [f"d{D}" for D in range(8, 89, 8)]
_NK = [f"nk{n}" for n in (2, 63, 64, 65, 127, 128, 129, 193)]
_NQ = [f"nq{n}" for n in (1, 31, 32, 33, 127, 128, 129)]
_BIAS = [f"bias_kh{kH}_nq{Nq}" for kH in (1, 2, 3) for Nq in (40, 129)]
_BH = ["b1h5", "b3h1", "b2h3"]
MUTATION_CASES = {
    "drop_last_key": _HEAD_DIMS + _NK + _NQ + _BIAS + _BH,
    "drop_first_key_of_last_tile": _HEAD_DIMS + _NK + _NQ + _BIAS + _BH,
    "swap_value_rows": _HEAD_DIMS + _NK + _NQ + _BIAS + _BH,
    "swap_head_scales": _BH,
    "p_unquantised": _HEAD_DIMS + _NK[1:] + _NQ + _BIAS + _BH,
    "denominator_row_d_minus_8": _HEAD_DIMS + _NK + _BH,
    "no_first_tile_rebase_below_7": _BIAS,
}


@pytest.mark.parametrize("mutation", list(MUTATION_CASES))
def test_the_element_bound_notices(mutation):
    """Each mutation is applied to the model (never to the kernel); the mutated output must leave the band bound + allowance of the GPU test around
    the unmutated model in at least one element, for every case listed."""
    for name in MUTATION_CASES[mutation]:
        c = F.CASES[name]
        x, M = F.case_model(name)
        W = F.model(x["q"], x["k"], x["v"], c.scale, x["rel_h"], x["rel_w"], mutation=mutation)
        band = F.element_bound(M) + M.allowance
        over = ~((W.out - M.out).abs() <= band)          # a NaN of the mutated model counts
        share = float(over.double().mean())
        print(f"{mutation} {name}: {100 * share:.2f} % of the elements over the band")
        assert share > 0, f"{mutation} goes unnoticed in case {name}"
