"""tests/geom_ref.py without a GPU.

a. The references against what they restate, to 1e-12 in float64: the MSDA forward against oracle.msda_ref and against
   F.grid_sample(align_corners=False, padding_mode="zeros"), its three gradients against float64 autograd through grid_sample away from
   cell boundaries and against oracle.msda_ref's backward (which returns fp32: to fp32 rounding; it has no "footprint outside" test, so
   its location gradient at exactly -1 px is left out of that comparison); postprocess against the F.interpolate -> crop -> F.interpolate
   chain; the positional encoding, preprocess and nms against oracle.sam_decoder_ref; the mask downscale against the F.conv2d /
   LayerNorm2d / GELU chain; the mask product against the permute-and-matmul statement.
b. The bounds against wrong kernels: per family the correctly rounded result (the same formulas in fp32, or the reference rounded to bf16)
   passes and each of a list of deliberately wrong results, made in torch at the sizes of the GPU cases, raises BoundFailure.
c. Conditions on the case data that the GPU tests rely on.
d. The case table names every `extern "C"` entry point of the two sources that anyedit_amd/_lib.py binds.
"""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import geom_ref as R
from geom_ref import BoundFailure

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSDA = R.CASES["ae_ms_deform_attn_bwd_f32"]
MSDA_SMALL = [c for c in MSDA if c["Q"] * c["d"] <= 2048]              # every level set, both reduction paths; the two Q = 300 cases left to (b), (c)


def fails(fn, *a, **kw):
    with pytest.raises(BoundFailure):
        fn(*a, **kw)


def close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert a.shape == b.shape and float((a.to(F64) - b.to(F64)).abs().max() if b.numel() else 0.0) <= tol * scale


@functools.lru_cache(maxsize=None)
def msda(i):
    cs = R.msda_case(MSDA[i])
    return cs, R.msda_reference(cs)


def idx(c):
    return MSDA.index(c)


# ====================================================================================================== a. references
@pytest.mark.parametrize("c", MSDA_SMALL, ids=str)
def test_msda_reference_equals_the_oracle(c):
    from oracle import msda_ref
    cs, ref = msda(idx(c))
    a = (cs.value.to(F64), cs.shapes, cs.starts, cs.loc.to(F64), cs.weight.to(F64))
    close(ref.out, msda_ref.ms_deform_attn(*a))
    gv, gl, gw = msda_ref.ms_deform_attn_backward(cs.value, cs.shapes, cs.starts, cs.loc, cs.weight, cs.grad_out)
    fp32 = 2.0 ** -22
    close(ref.gv, gv, fp32)
    close(ref.gw, gw, fp32)
    at_minus_one = torch.zeros_like(ref.outside)
    for l in range(cs.dims[5]):
        x, y = R.msda_coords(cs, l)[:2]
        at_minus_one[:, :, :, l, :] = (x == -1) | (y == -1)
    keep = ~at_minus_one[..., None].expand_as(gl)
    close(ref.gl[0][keep], gl[keep], fp32)
    assert bool((ref.gl[0][~keep] == 0).all())


@pytest.mark.parametrize("c", MSDA_SMALL, ids=str)
def test_msda_reference_equals_grid_sample_and_its_autograd(c):
    cs, ref = msda(idx(c))
    bs, S, heads, d, Q, L, P = cs.dims
    value, loc, w = (t.to(F64).requires_grad_(True) for t in (cs.value, cs.loc, cs.weight))
    out = torch.zeros(bs, heads, d, Q, dtype=F64)
    smooth = torch.ones(bs, Q, heads, L, P, dtype=torch.bool)
    for l in range(L):
        H, W = (int(v) for v in cs.shapes[l])
        s0 = int(cs.starts[l])
        img = value[:, s0:s0 + H * W].permute(0, 2, 3, 1).reshape(bs * heads, d, H, W)
        grid = (2.0 * loc[:, :, :, l] - 1.0).permute(0, 2, 1, 3, 4).reshape(bs * heads, Q, P, 2)
        samp = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)      # [bs heads, d, Q, P]
        out = out + (samp * w[:, :, :, l].permute(0, 2, 1, 3).reshape(bs * heads, 1, Q, P)).sum(-1).reshape(bs, heads, d, Q)
        x, y = R.msda_coords(cs, l)[:2]
        smooth[:, :, :, l, :] = ((x - x.round()).abs() > 1e-6) & ((y - y.round()).abs() > 1e-6)
    out = out.permute(0, 3, 1, 2).reshape(bs, Q, heads * d)
    close(ref.out, out.detach())
    gv, gl, gw = torch.autograd.grad(out, (value, loc, w), cs.grad_out.to(F64))
    close(ref.gv, gv)
    close(ref.gw, gw)
    m = smooth[..., None].expand_as(gl)
    close(ref.gl[0][m], gl[m])
    assert int(smooth.sum()) > 0 or smooth.numel() == 1     # the one sample of the 1 x 1 case is the pixel's centre


@pytest.mark.parametrize("c", R.CASES["ae_sam_postprocess_masks"][::5], ids=str)
def test_postprocess_reference_equals_the_interpolate_chain(c):
    from oracle import sam_decoder_ref as SD
    low = R.postprocess_case(c)
    ref, _ = R.ref_postprocess(low, c["S"], *c["inp"], *c["orig"])
    close(ref, SD.postprocess_masks(low.to(F64)[None], c["S"], c["inp"], c["orig"])[0])


@pytest.mark.parametrize("c", R.CASES["ae_sam_pe_encode_f32"][::5], ids=str)
def test_pe_reference_equals_the_oracle(c):
    from oracle import sam_decoder_ref as SD
    xy, gauss, labels, table = R.pe_case(c)
    ref, _ = R.ref_pe(xy, gauss, c["H"], c["W"], c["offset"])
    c01 = (xy.to(F64) + R.c32(c["offset"])) * torch.tensor([R.c32(1.0 / c["W"]), R.c32(1.0 / c["H"])], dtype=F64)
    close(ref, SD.pe_encoding(gauss.to(F64), c01))
    if labels is not None and c["offset"] == 0.5:             # embed_points adds its own 0.5 and runs in fp32; labels -1, 0, 1 only
        Fq = gauss.shape[1]
        sd = {"prompt_encoder.pe_layer.positional_encoding_gaussian_matrix": gauss, "prompt_encoder.not_a_point_embed.weight": table[0:1],
              "prompt_encoder.point_embeddings.0.weight": table[1:2], "prompt_encoder.point_embeddings.1.weight": table[2:3]}
        sel = labels <= 1
        want = SD.embed_points(sd, xy[sel][None], labels[sel][None], False, (c["H"], c["W"]))[0]
        got, bnd = R.ref_pe(xy, gauss, c["H"], c["W"], 0.5, labels, table)
        assert got[sel].shape == (int(sel.sum()), 2 * Fq)
        assert R.check_elements(want, got[sel], bnd[sel], "the oracle's fp32 result meets the kernel's bound") <= 1.0


@pytest.mark.parametrize("c", R.CASES["ae_sam_preprocess_f32"], ids=str)
def test_preprocess_reference_equals_the_oracle(c):
    from oracle import sam_decoder_ref as SD
    x, mean, std = R.preprocess_case(c)
    ref, _, pad = R.ref_preprocess(x, c["S"], mean, std)
    close(ref, SD.preprocess(x.to(F64), c["S"], mean.to(F64), std.to(F64)))
    assert bool((ref[pad] == 0).all()) and int((~pad).sum()) == x.numel()


def test_nms_reference_equals_the_oracle():
    from oracle import sam_decoder_ref as SD
    for c in R.CASES["ae_nms_sorted_f32"]:
        if c.get("N", 0) > 257 or c["kind"] == "zero_area":      # the oracle is a Python double loop, and divides 0 by 0
            continue
        boxes = R.nms_case(c)
        scores = -torch.arange(boxes.shape[0], dtype=F32)
        keep = R.ref_nms(boxes, c["thr"])
        assert keep.nonzero().flatten().tolist() == SD.nms(boxes, scores, R.c32(c["thr"])).tolist(), c
    built = {k: R.ref_nms(R.nms_case(dict(kind=k)), 0.5).tolist() for k in ("tie", "duplicates", "zero_area", "chain", "equal_scores")}
    assert built == {"tie": [1, 1, 1, 1, 1], "duplicates": [1, 0, 1, 0, 0], "zero_area": [1, 1, 1, 1, 0, 1], "chain": [1, 0, 1],
                     "equal_scores": [1, 0, 1, 0, 0]}


@pytest.mark.parametrize("c", R.CASES["ae_sam_mask_downscale_bf16"], ids=str)
def test_mask_downscale_reference_equals_the_conv_layernorm_gelu_chain(c):
    m, p = R.downscale_case(c)
    q = {k: v.to(F64) for k, v in p.items()}

    def ln2d(x, g, b):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return g[:, None, None] * ((x - u) / torch.sqrt(s + R.c32(1e-6))) + b[:, None, None]
    h = F.gelu(ln2d(F.conv2d(m.to(F64), q["w1"], q["b1"], stride=2), q["g1"], q["e1"]))
    h = F.gelu(ln2d(F.conv2d(h, q["w2"], q["b2"], stride=2), q["g2"], q["e2"]))
    close(R.ref_mask_downscale(m, p)[0], h.permute(0, 2, 3, 1).reshape(-1, 16))


@pytest.mark.parametrize("c", R.CASES["ae_sam_mask_product_f32"][3::7], ids=str)
def test_mask_product_reference_equals_permute_and_matmul(c):
    up, hyper = R.product_case(c)
    B, C, M, h, w = c["B"], c["C"], c["M"], c["h"], c["w"]
    img = up.to(F64).reshape(B, h, w, 2, 2, 2, 2, C).permute(0, 7, 1, 3, 5, 2, 4, 6).reshape(B, C, 4 * h, 4 * w)
    close(R.ref_mask_product(up, hyper, B, h, w)[0], (hyper.to(F64) @ img.reshape(B, C, -1)).reshape(B, M, 4 * h, 4 * w))


# ====================================================================================================== b. wrong kernels
WRONG_ON = {"out": ("swap_xy", "swap_wh", "align_corners", "clamp_rim", "drop_corner", "level_row"), "gv": ("swap_xy", "drop_corner", "level_row"),
            "gl": ("swap_xy", "swap_wh", "align_corners", "clamp_rim", "drop_corner", "no_wh"), "gw": ("swap_wh", "clamp_rim", "drop_corner", "gw_times_w")}


@pytest.mark.parametrize("c", [MSDA[4], MSDA[6], MSDA[7], MSDA[8]], ids=str)
def test_msda_bounds_accept_fp32_and_reject_wrong_kernels(c):
    cs, ref = msda(idx(c))
    ok = R.msda_eval(cs, F32)
    r = R.msda_check(ref, ok.out, ok.gv, ok.gl, ok.gw)
    assert max(r.values()) <= 1.0
    seen = set()
    for name in ("out", "gv", "gl", "gw"):
        for wrong in WRONG_ON[name]:
            if wrong == "swap_wh" and all(h == w for h, w in c["levels"]):
                continue                                       # square levels: the same kernel
            bad = R.msda_eval(cs, F32, wrong=wrong)
            fails(R.msda_check, ref, **{name: getattr(bad, name)})
            seen.add(wrong)
    assert seen | {"swap_wh"} == set(R.MSDA_WRONG)
    # a sample outside must give exactly 0: the smallest nonzero fails
    gw = ok.gw.clone()
    assert bool(ref.outside.any())
    gw[ref.outside] = 1e-30
    fails(R.msda_check, ref, gw=gw)


def test_msda_cell_rule_allows_either_neighbour_only_where_fp32_is_inexact():
    cs, ref = msda(7)                                          # power-of-two levels: pixel centres are exact, floor's cell is required
    centre = cs.klass == cs.c["classes"].index("centre")
    assert ref.alts == [(0, 0)] or not any(bool(R.msda_coords(cs, l)[4][centre[:, :, :, l]].any()) for l in range(4))
    left = R.msda_eval(cs, F64, alt=(0, 0)).gl.clone()
    # the gradient of the cell to the left / above at a pixel centre: what a kernel that floors x - tiny would return
    x, y, _, _, _, _ = R.msda_coords(cs, 0)
    forced = R.types.SimpleNamespace(**vars(cs))
    forced.loc = cs.loc.clone()
    forced.loc[:, :, :, 0][centre[:, :, :, 0]] -= 2.0 ** -12   # 2^-12 of the frame = 2^-9 px into the left / upper cell of the 8 x 8 level
    other = R.msda_eval(forced, F64).gl
    assert float((other - left)[:, :, :, 0][centre[:, :, :, 0]].abs().max()) > 1e-3
    left[:, :, :, 0][centre[:, :, :, 0]] = other[:, :, :, 0][centre[:, :, :, 0]]
    fails(R.msda_check, ref, gl=left)
    cs2, ref2 = msda(6)                                        # 13 x 17 ...: a centre is within e_c of an integer, either cell passes
    assert len(ref2.alts) == 4
    for e in (R.msda_eval(cs2, F64, alt=a) for a in ref2.alts):
        assert R.msda_check(ref2, gl=e.gl)["grad_loc"] <= 1.0


def test_linear_bound_accepts_fp32_and_rejects_bf16_inputs_and_a_dropped_bias():
    for c in R.CASES["ae_linear_f32"]:
        if (c["M"], c["bias"]) != (65, 1):
            continue
        x, w, b = R.linear_case(c)
        ref, bnd = R.ref_linear(x, w, b)
        acc = torch.zeros(c["M"], c["N"], dtype=F32)
        for k in range(c["K"]):                                # an fp32 chain in k order, then the bias
            acc = acc + x[:, k:k + 1] * w[:, k][None]
        assert R.check_elements(acc + b, ref, bnd, "fp32") <= 1.0
        assert R.check_elements(x @ w.t() + b, ref, bnd, "fp32 blocked") <= 1.0
        fails(R.check_elements, x.to(BF).float() @ w.to(BF).float().t() + b, ref, bnd, "bf16 inputs")
        bad = (x @ w.t() + b).clone()
        bad[:, (c["N"] - 1) // 64 * 64:] -= b[(c["N"] - 1) // 64 * 64:]
        fails(R.check_elements, bad, ref, bnd, "bias dropped on the last column tile")


def test_pe_bound_accepts_fp32_and_rejects_swapped_scales_and_wrong_label_rows():
    for c in R.CASES["ae_sam_pe_encode_f32"]:
        if not c["labels"] or c["N"] == 1:
            continue
        xy, gauss, labels, table = R.pe_case(c)
        ref, bnd = R.ref_pe(xy, gauss, c["H"], c["W"], c["offset"], labels, table)
        off, iw, ih = (torch.tensor(R.c32(v), dtype=F32) for v in (c["offset"], 1.0 / c["W"], 1.0 / c["H"]))
        x, y = (xy[:, 0] + off) * iw, (xy[:, 1] + off) * ih
        ph = ((2 * x - 1)[:, None] * gauss[0] + (2 * y - 1)[:, None] * gauss[1]) * torch.tensor(6.283185307179586, dtype=F32)
        enc = torch.cat([torch.sin(ph), torch.cos(ph)], 1)
        enc[labels < 0] = 0.0
        got = enc + table[torch.where(labels < 0, 0, 1 + labels).long()]
        assert R.check_elements(got, ref, bnd, "fp32") <= 1.0
        if c["H"] != c["W"]:
            fails(R.check_elements, R.ref_pe(xy, gauss, c["H"], c["W"], c["offset"], labels, table, "swap_inv")[0], ref, bnd, "inv_w / inv_h exchanged")
        fails(R.check_elements, R.ref_pe(xy, gauss, c["H"], c["W"], c["offset"], labels, table, "row_off")[0], ref, bnd, "label row off by one")
        fails(R.check_elements, R.ref_pe(xy, gauss, c["H"], c["W"], c["offset"], labels, table, "keep_neg")[0], ref, bnd, "label -1 keeps the encoding")


def test_mask_product_bound_accepts_fp32_and_rejects_a_wrong_unshuffle_and_batch():
    for c in R.CASES["ae_sam_mask_product_f32"]:
        if (c["h"], c["w"]) != (5, 7) or c["B"] != 3:
            continue
        up, hyper = R.product_case(c)
        a = (up, hyper, c["B"], c["h"], c["w"])
        ref, bnd = R.ref_mask_product(*a)
        assert R.check_elements(ref.float(), ref, bnd, "fp32") <= 1.0
        fails(R.check_elements, R.ref_mask_product(*a, "swap_dy")[0].float(), ref, bnd, "dy1 / dy2 exchanged")
        fails(R.check_elements, R.ref_mask_product(*a, "wrong_batch")[0].float(), ref, bnd, "hyper row of another batch")


def test_postprocess_bound_accepts_fp32_and_rejects_wrong_resampling():
    rejected = {"no_crop": 0, "align_corners": 0, "unclamped": 0}
    for c in R.CASES["ae_sam_postprocess_masks"]:
        if c["mode"] != "both":
            continue
        low = R.postprocess_case(c)
        a = (low, c["S"], *c["inp"], *c["orig"])
        ref, bnd = R.ref_postprocess(*a)
        chain = F.interpolate(low[None], (c["S"], c["S"]), mode="bilinear", align_corners=False)[..., :c["inp"][0], :c["inp"][1]]
        got = F.interpolate(chain, tuple(c["orig"]), mode="bilinear", align_corners=False)[0]
        assert R.check_elements(got, ref, bnd, "fp32") <= 1.0
        mask, decided = R.postprocess_mask(ref, bnd, c["thr"], False)
        assert R.check_mask((got > c["thr"]).to(torch.uint8), mask, decided, "mask") == 0.0
        fails(R.check_mask, 1 - mask, mask, decided, "inverted")
        for v in rejected:
            bad = R.ref_postprocess(*a, v)[0].float()
            if not torch.equal(bad, ref.float()):              # a geometry without padding has no crop; one at scale 1 has no upper neighbour
                fails(R.check_elements, bad, ref, bnd, v)
                rejected[v] += 1
    assert min(rejected.values()) >= 2, rejected


def test_mask_downscale_bound_accepts_bf16_and_rejects_unbiased_variance_and_tanh_gelu():
    for c in R.CASES["ae_sam_mask_downscale_bf16"]:
        m, p = R.downscale_case(c)
        ref, bnd = R.ref_mask_downscale(m, p)
        assert R.check_elements(ref.to(BF), ref, bnd, "bf16") <= 1.0
        if c["h"] * c["w"] < 100:
            continue
        fails(R.check_elements, R.ref_mask_downscale(m, p, variant="unbiased")[0].to(BF), ref, bnd, "unbiased variance")
        fails(R.check_elements, R.ref_mask_downscale(m, p, variant="tanh")[0].to(BF), ref, bnd, "tanh GELU")
        fails(R.check_elements, ref.to(BF).roll(1, 0), ref, bnd, "the neighbour's pixel")


def test_nms_and_preprocess_checks_reject_wrong_results():
    tie, chain = R.nms_case(dict(kind="tie")), R.nms_case(dict(kind="chain"))
    fails(R.check_bits, R.ref_nms(tie, 0.5, "ge"), R.ref_nms(tie, 0.5), ">= instead of >")
    fails(R.check_bits, R.ref_nms(chain, 0.5, "by_removed"), R.ref_nms(chain, 0.5), "suppression by a removed box")
    big = R.nms_case(R.CASES["ae_nms_sorted_f32"][8])
    assert big.shape[0] == 3855
    fails(R.check_bits, R.ref_nms(big, 0.3, "by_removed"), R.ref_nms(big, 0.3), "suppression by a removed box, random boxes")
    c = R.CASES["ae_sam_preprocess_f32"][0]
    x, mean, std = R.preprocess_case(c)
    ref, bnd, pad = R.ref_preprocess(x, c["S"], mean, std)
    ok = F.pad((x - mean.reshape(-1, 1, 1)) / std.reshape(-1, 1, 1), (0, c["S"] - c["w"], 0, c["S"] - c["h"]))
    assert R.check_elements(ok, ref, bnd, "fp32") <= 1.0
    fails(R.check_elements, F.pad((x - mean.reshape(-1, 1, 1)) * (1.0 / std).to(BF).float().reshape(-1, 1, 1), (0, c["S"] - c["w"], 0, c["S"] - c["h"])),
          ref, bnd, "a bf16 reciprocal")
    fails(R.check_elements, ok + 1e-20 * pad, ref, bnd, "padding not zero")


# ====================================================================================================== c. conditions on the case data
def test_postprocess_cases_leave_at_most_a_thousandth_of_the_pixels_undecided():
    for c in R.CASES["ae_sam_postprocess_masks"]:
        ref, bnd = R.ref_postprocess(R.postprocess_case(c), c["S"], *c["inp"], *c["orig"])
        _, decided = R.postprocess_mask(ref, bnd, c["thr"], c["mode"] == "merge")
        assert int((~decided).sum()) <= 1e-3 * decided.numel(), c


def test_random_nms_cases_have_no_iou_near_the_threshold():
    for c in R.CASES["ae_nms_sorted_f32"]:
        if c["kind"] != "random":
            continue
        boxes, t = R.nms_case(c), R.c32(c["thr"])
        worst = 1.0
        for r0 in range(0, boxes.shape[0], 512):
            iou = R.nms_iou(boxes, torch.arange(r0, min(r0 + 512, boxes.shape[0])))
            worst = min(worst, float((iou / t - 1.0).abs().min()))
        assert worst > 2.0 ** -20, c
        if c["N"] > 2:
            keep = R.ref_nms(boxes, c["thr"])
            assert 0 < int(keep.sum()) < c["N"], "some boxes fall, some stay"


@pytest.mark.parametrize("c", MSDA, ids=str)
def test_msda_cases_contain_the_location_classes_they_claim(c):
    cs = R.msda_case(c)
    bs, S, heads, d, Q, L, P = cs.dims
    assert bool((cs.weight == 0).any()) or cs.weight.numel() < 5
    assert cs.weight.numel() < 3 or (bool((cs.weight < 0).any()) and bool((cs.weight > 0).any()))
    for l in range(L):
        H, W = (int(v) for v in cs.shapes[l])
        x, y, ecx, ecy, nx, ny = R.msda_coords(cs, l)
        lx, ly = cs.loc[:, :, :, l, :, 0], cs.loc[:, :, :, l, :, 1]
        inx, iny = (x >= 0) & (x <= W - 1), (y >= 0) & (y <= H - 1)
        rimx, rimy = ((x > -1) & (x < 0)) | ((x > W - 1) & (x < W)), ((y > -1) & (y < 0)) | ((y > H - 1) & (y < H))
        outx, outy = (x <= -1) | (x >= W), (y <= -1) | (y >= H)
        is_class = {
            "inside": inx & iny,
            "frame": (lx == 0) | (lx == 1) | (ly == 0) | (ly == 1),
            "rim1": rimx & rimy,
            "rim2": (rimx & iny) | (inx & rimy),
            "edge": (outx & (torch.minimum((x + 1).abs(), (x - W).abs()) < 1e-4)) | (outy & (torch.minimum((y + 1).abs(), (y - H).abs()) < 1e-4)),
            "far": (x < -2) | (x > W + 1) | (y < -2) | (y > H + 1),
            "centre": ((x - x.round()).abs() <= ecx) & ((y - y.round()).abs() <= ecy) & inx & iny,
        }
        k = cs.klass[:, :, :, l, :]
        for ci, name in enumerate(c["classes"]):
            mine = k == ci
            assert bool(mine.any()), (name, l)
            assert bool(is_class[name][mine].all()), (name, l)
        # a sample that is outside in float64 is outside in fp32 too: exactly on the edge where fp32 is exact, else two allowances beyond it
        for o, v, n, e in ((outx, x, W, ecx), (outy, y, H, ecy)):
            past = torch.where(v <= -1, -1 - v, v - n)[o]
            assert bool(((past >= 2 * e[o]) | ((past == 0) & R.pow2(n))).all()), l
        if c.get("only"):
            assert bool((outx | outy).all())
    assert cs.shuffle == (d in (4, 8, 32, 256))


def test_msda_cases_cover_the_sizes_the_kernels_branch_on():
    cs = MSDA
    assert {c["d"] for c in cs} >= {4, 8, 32, 256, 12, 20} and {c["heads"] for c in cs} >= {1, 3, 8} and {c["bs"] for c in cs} == {1, 2}
    assert {c["Q"] for c in cs} >= {1, 7, 300} and {(len(c["levels"]), c["P"]) for c in cs} >= {(1, 1), (2, 3), (4, 4)}
    totals = {c["bs"] * c["Q"] * c["heads"] * (c["d"] // 4) for c in cs}
    assert {63, 256 + 64 + 8} <= totals
    both_paths_all_outside = {R.msda_case(c).shuffle for c in cs if c.get("only")}
    assert both_paths_all_outside == {True, False}


# ====================================================================================================== d. the case table is complete
def test_every_entry_point_of_the_two_sources_has_a_case():
    from anyedit_amd import _lib
    exported = set()
    for src in R.SOURCES:
        with open(os.path.join(ROOT, "anyedit_amd", "csrc", src)) as f:
            exported |= set(re.findall(r'extern "C" int (ae_\w+)\(', f.read()))
    assert len(exported) == 9
    assert exported - set(_lib.SIGNATURES) == set(), f"exported but not bound: {sorted(exported - set(_lib.SIGNATURES))}"
    assert exported == set(R.CASES), f"without a case: {sorted(exported - set(R.CASES))}; cases without an entry point: {sorted(set(R.CASES) - exported)}"
    assert all(len(v) > 0 for v in R.CASES.values())
