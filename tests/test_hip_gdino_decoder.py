"""GPU tests of the device code of GroundingDINO's query selection, decoder and heads (anyedit_amd/csrc/gdino_decoder.hip): every kernel writes
into sentinel-filled buffers between guard bands (through a row stride wider than the row where it takes one), is launched twice and must give
bit-identical outputs.  Every case runs once.

Bounds, each from the arithmetic and not from what the kernels give:
  contrastive   every finite logit within 2^-15 * sum_i |x_i y_i| + 1e-30 of float64 on the same bf16 inputs (<= 256 fp32 accumulations of exact
                products at one fp32 ulp each, in any order); the -inf pattern exact; rowmax bit-equal to the row maximum of the logits of the
                same call.
  top-k         exact equality with the stable descending sort computed on the CPU from the same values.
  proposals     flags and inf pattern exact; finite values within 2^-19 * max(1, |ref|) of the fp32 reference (one rounding of the quotient and a
                few ulps of logf at |value| <= 4.6).
  query sine    reference_points_input bit-equal to the fp32 product; the embedding within 2^-8 |ref| + 2^-18 of float64 (one bf16 rounding plus
                three fp32 roundings of an argument <= 2 pi).
  box refine    u within 2^-15 * (sum |h_i w_i| + |b|) + 2^-20 * (1 + |u_ref|) of the fp32 torch formula, sigmoid(u) within a quarter of that
                plus 2^-22.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, T  # noqa: E402
import gdino_dec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
GUARD = 4096
SENT_BYTE = 0xFF                       # as fp32 and as bf16 a NaN no kernel writes, as an index -1
SENT_F32 = -1                          # int32 view of four sentinel bytes
SENT_BF = -1                           # int16 view of two
INF = float("inf")


class Guarded:
    """A tensor of `shape` / `dtype` inside a byte buffer filled with 0xFF, with GUARD bytes of the same before and after it."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((n + 2 * GUARD,), SENT_BYTE, dtype=torch.uint8, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(*shape)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT_BYTE).all()) and bool((self.buf[-GUARD:] == SENT_BYTE).all())


def _twice(fn):
    """fn() -> (list of Guarded outputs); runs it twice, checks the guards, requires bit-identical buffers, returns the first run's tensors on the CPU."""
    runs = []
    for _ in range(2):
        outs = fn()
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs), "wrote outside its outputs"
        runs.append([o.t.clone().cpu() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), "two launches differ"
    return runs[0]


# ------------------------------------------------------------------------------------------------------------------ contrastive
def _token_masks(kind, B, Tn, gen):
    if kind == "none":
        return None
    m = torch.ones(B, Tn, dtype=torch.bool)
    if kind == "random":
        m = torch.rand(B, Tn, generator=gen) < 0.6
        for b in range(B):
            m[b, int(torch.randint(Tn, (1,), generator=gen))] = True
    elif kind == "one":                 # all but one token unused, a different one per sample
        m[:] = False
        for b in range(B):
            m[b, (b * 5 + Tn // 2) % Tn] = True
    elif kind == "empty1":              # sample 1 has no used token: everything -inf
        m = torch.rand(B, Tn, generator=gen) < 0.6
        m[0, 0] = True
        m[1] = False
    return m


def _contrastive_case(N, Tn, L, C, kind, mode, seed):
    from anyedit_amd import ops
    B = 2
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, C, generator=gen).to(BF)
    y = torch.randn(B, Tn, C, generator=gen).to(BF)
    m = _token_masks(kind, B, Tn, gen)
    ldx, ldl = C + 8, L + 4
    xw = torch.full((B, N, ldx), float("nan"), dtype=BF)
    xw[..., :C] = x
    dx, dy = xw.to(DEV)[..., :C], y.to(DEV)
    dm = None if m is None else m.to(DEV)
    want_l, want_r = mode in ("both", "logits"), mode in ("both", "rowmax")

    def run():
        gl, gr = Guarded((B, N, ldl), torch.float32), Guarded((B, N), torch.float32)
        lo, ro = ops.contrastive(dx, dy, dm, max_text_len=L, want_logits=want_l, want_rowmax=want_r, logits=gl.t[..., :L] if want_l else None,
                                 rowmax=gr.t if want_r else None)
        assert (lo is None) == (not want_l) and (ro is None) == (not want_r)
        return [gl, gr]

    lw, rm = _twice(run)
    mm = torch.ones(B, Tn, dtype=torch.bool) if m is None else m
    ref = R.contrastive(x.to(F64), y.to(F64), mm, L)
    mag = R.contrastive(x.to(F64).abs(), y.to(F64).abs(), mm, L)
    worst = 0.0
    if want_l:
        assert bool((lw[..., L:].contiguous().view(torch.int32) == SENT_F32).all()), "columns between max_text_len and the row stride must stay untouched"
        got = lw[..., :L]
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isneginf(got), ~fin), "-inf pattern"
        worst = float(((got.to(F64) - ref)[fin].abs() / (2.0 ** -15 * mag[fin] + 1e-30)).max()) if fin.any() else 0.0
    else:
        assert bool((lw.view(torch.int32) == SENT_F32).all()), "a rowmax-only call must not write logits"
    if want_r:
        rref = ref.max(-1)[0]
        assert torch.equal(torch.isneginf(rm), torch.isneginf(rref))
        if want_l:
            assert torch.equal(rm.view(torch.int32), lw[..., :L].max(-1)[0].contiguous().view(torch.int32)), "rowmax is not the maximum of the call's own logits"
        else:
            fin = torch.isfinite(rref)
            # the maximum of values each within its bound of the reference is within the largest bound of the row of the reference maximum
            bound = 2.0 ** -15 * torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)).max(-1)[0] + 1e-30
            worst = max(worst, float(((rm.to(F64) - rref)[fin].abs() / bound[fin]).max()) if fin.any() else 0.0)
    else:
        assert bool((rm.view(torch.int32) == SENT_F32).all()), "a logits-only call must not write rowmax"
    print(f"contrastive N={N} T={Tn} max_text_len={L} C={C} mask={kind} mode={mode}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("N", [1, 63, 65, 130])
@pytest.mark.parametrize("Tn,L", [(1, 1), (1, 256), (17, 17), (17, 256), (255, 255), (255, 256), (256, 256)])
def test_contrastive_vs_float64_over_rows_and_tokens(N, Tn, L, C):
    _contrastive_case(N, Tn, L, C, "random", "both", 100 * N + Tn + L + C)


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("kind", ["none", "random", "one", "empty1"])
@pytest.mark.parametrize("mode", ["both", "rowmax", "logits"])
def test_contrastive_masks_and_output_modes(C, kind, mode):
    _contrastive_case(65, 17, 256 if mode != "rowmax" else 17, C, kind, mode, 7 + C)


def test_contrastive_reproduces_the_reference_fixture():
    from anyedit_amd import ops
    z = load_golden("gdino_dec_geom")
    x, y, m = T(z["ce_x"]).to(BF), T(z["ce_y"]).to(BF), T(z["ce_mask"])
    got, _ = ops.contrastive(x.to(DEV), y.to(DEV), m.to(DEV), max_text_len=16)
    ref = T(z["ce_out"])
    assert torch.equal(torch.isneginf(got.cpu()), torch.isneginf(ref))
    mine = R.contrastive(x.to(F64), y.to(F64), m, 16)          # the fixture's fp32 inputs rounded to bf16, as the kernel reads them
    mag = R.contrastive(x.to(F64).abs(), y.to(F64).abs(), m, 16)
    fin = torch.isfinite(ref)
    assert bool(((got.cpu().to(F64) - mine)[fin].abs() <= 2.0 ** -15 * mag[fin] + 1e-30).all())


def test_contrastive_refusals():
    from anyedit_amd import ops
    x = torch.zeros(1, 4, 64, dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.contrastive(torch.zeros(1, 4, 48, dtype=BF, device=DEV), torch.zeros(1, 3, 48, dtype=BF, device=DEV))
    with pytest.raises(ValueError, match="max_text_len"):
        ops.contrastive(x, torch.zeros(1, 257, 64, dtype=BF, device=DEV))
    with pytest.raises(ValueError, match="max_text_len"):
        ops.contrastive(x, torch.zeros(1, 8, 64, dtype=BF, device=DEV), max_text_len=7)
    with pytest.raises(ValueError, match="neither"):
        ops.contrastive(x, torch.zeros(1, 8, 64, dtype=BF, device=DEV), want_logits=False)


# ------------------------------------------------------------------------------------------------------------------ top-k
def _topk_values(kind, B, N, k, gen):
    v = torch.randn(B, N, generator=gen)
    if kind == "normal":
        return v
    if kind == "quantised":             # 8 levels: tie runs far longer than a thread's slice, across every slice boundary
        return torch.floor(v.clamp(-2, 1.99) * 2) / 2
    if kind == "equal":
        return torch.full((B, N), 0.25)
    if kind == "neg_inf":               # fewer than k finite entries: -inf entries are selected, lowest index first
        keep = max(0, k - 1 - max(1, k // 3))
        for b in range(B):
            idx = torch.randperm(N, generator=gen)[keep:] if keep else torch.arange(N)
            v[b, idx] = -INF
        return v
    if kind == "zeros":                 # -0.0 and +0.0 are one value
        z = torch.zeros(B, N)
        z[torch.rand(B, N, generator=gen) < 0.5] = -0.0
        sel = torch.rand(B, N, generator=gen) < 0.7
        return torch.where(sel, z, v)
    if kind == "pos_inf":
        v[torch.rand(B, N, generator=gen) < 0.2] = INF
        return v
    if kind == "nan":                   # NaN of either sign orders above +inf
        r = torch.rand(B, N, generator=gen)
        v[r < 0.15] = float("nan")
        bits = v.view(torch.int32)
        bits[(r >= 0.15) & (r < 0.3)] = -4194304        # 0xFFC00000: the negative quiet NaN
        v[(r >= 0.3) & (r < 0.4)] = INF
        v[(r >= 0.4) & (r < 0.45)] = -INF
        return v
    raise ValueError(kind)


@pytest.mark.parametrize("N,k", [(1, 1), (7, 7), (301, 300), (1000, 1), (13294, 900), (70001, 1024)])
@pytest.mark.parametrize("kind", ["normal", "quantised", "equal", "neg_inf", "zeros", "pos_inf", "nan"])
def test_topk_rows_is_the_stable_descending_sort(N, k, kind):
    from anyedit_amd import ops
    B = 3
    gen = torch.Generator().manual_seed(N * 31 + k + len(kind))
    v = _topk_values(kind, B, N, k, gen)
    ld = N + 5
    vw = torch.full((B, ld), INF)       # the pad columns would win every selection if they were read
    vw[:, :N] = v
    dv = vw.to(DEV)[:, :N]

    def run():
        g = Guarded((B, k), torch.int32)
        assert ops.topk_rows(dv, k, out=g.t).data_ptr() == g.t.data_ptr()
        return [g]

    got, = _twice(run)
    ref = R.stable_topk(v, k).to(torch.int32)
    same = torch.equal(got, ref)
    print(f"topk N={N} k={k} {kind}: equal {same}")
    assert same, f"first differing slots: {(got != ref).nonzero()[:4].tolist()}"


def test_topk_rows_refusals():
    from anyedit_amd import ops
    v = torch.zeros(2, 2000, device=DEV)
    with pytest.raises(ValueError, match="k=1025"):
        ops.topk_rows(v, 1025)
    with pytest.raises(ValueError, match="k=8"):
        ops.topk_rows(v[:, :7], 8)
    with pytest.raises(ValueError, match="k=0"):
        ops.topk_rows(v, 0)
    assert ops.topk_rows_max_n() >= 1 << 20


# ------------------------------------------------------------------------------------------------------------------ proposals
def _proposals_case(mask, levels, ref, ref_keep):
    from anyedit_amd import ops
    B, N = mask.shape
    dm = mask.to(DEV)

    def run():
        gp, gk = Guarded((B, N, 4), torch.float32), Guarded((B, N), torch.uint8)
        ops.gdino_proposals(dm, levels, proposals=gp.t, keep=gk.t)
        return [gp, gk]

    got, keep = _twice(run)
    assert torch.equal(keep.bool(), ref_keep), "keep flags"
    assert torch.equal(torch.isposinf(got), torch.isposinf(ref)) and not torch.isnan(got).any() and not torch.isneginf(got).any(), "inf pattern"
    fin = torch.isfinite(ref)
    assert torch.equal(fin.all(-1), ref_keep) and torch.equal(fin.any(-1), ref_keep)
    worst = float(((got - ref)[fin].abs().double() / (2.0 ** -19 * ref[fin].abs().clamp(min=1.0).double())).max()) if fin.any() else 0.0
    print(f"proposals levels={levels} B={B}: kept {int(ref_keep.sum())} of {ref_keep.numel()}, worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


def test_proposals_reproduce_the_reference_fixture():
    z = load_golden("gdino_dec_geom")
    levels = [tuple(int(v) for v in hw) for hw in z["spatial_shapes"]]
    assert (1, 1) in levels
    mask, ref, kept = T(z["padding_mask"]), T(z["proposals"]), T(z["memory_kept"])
    _proposals_case(mask, levels, ref, kept)
    mine, keep = R.encoder_output_proposals(mask, levels)
    assert torch.equal(keep, kept) and torch.equal(torch.isfinite(mine), torch.isfinite(ref))


@pytest.mark.parametrize("levels", [[(1, 1)], [(100, 133), (50, 67), (25, 34), (13, 17)], [(1, 1), (3, 300), (17, 2)]])
def test_proposals_vs_restatement_with_a_fully_padded_sample(levels):
    gen = torch.Generator().manual_seed(len(levels) + levels[0][0])
    B, N = 4, sum(h * w for h, w in levels)
    mask = torch.zeros(B, N, dtype=torch.bool)
    s = 0
    for H, W in levels:
        a = torch.ones(H, W, dtype=torch.bool)
        a[:max(1, (2 * H) // 3), :max(1, (3 * W) // 4)] = False
        mask[1, s:s + H * W] = a.reshape(-1)
        mask[3, s:s + H * W] = torch.rand(H * W, generator=gen) < 0.5      # not a rectangle: only the first row / column count
        s += H * W
    mask[2] = True                       # fully padded: valid extents 0, every proposal +inf, no fault
    ref, keep = R.encoder_output_proposals(mask, levels)
    assert not keep[2].any() and bool(torch.isposinf(ref[2]).all())
    _proposals_case(mask, levels, ref, keep)


def test_proposals_refusals():
    from anyedit_amd import ops
    m = torch.zeros(1, 12, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="do not tile"):
        ops.gdino_proposals(m, [(3, 3)])
    with pytest.raises(ValueError, match="do not tile"):
        ops.gdino_proposals(m, [(1, 1)] * 12)


# ------------------------------------------------------------------------------------------------------------------ query sine
@pytest.mark.parametrize("nq", [1, 20, 900])
@pytest.mark.parametrize("L", [1, 4])
def test_query_sine_vs_float64(nq, L):
    from anyedit_amd import ops
    B = 2
    gen = torch.Generator().manual_seed(nq + L)
    ref = torch.rand(B, nq, 4, generator=gen)
    ref[0, 0] = torch.tensor([0.0, 1.0, 0.5, 0.0])
    ref[1, nq - 1] = torch.tensor([1.0, 0.0, 1.0, 1.0])
    vr = 0.5 + 0.5 * torch.rand(B, L, 2, generator=gen)
    vr[0] = 1.0
    dr, dv = ref.to(DEV), vr.to(DEV)
    lde = 512 + 8

    def run():
        gi, ge = Guarded((B, nq, L, 4), torch.float32), Guarded((B * nq, lde), BF)
        ops.gdino_query_sine(dr, dv, ref_input=gi.t, embed=ge.t[:, :512])
        return [gi, ge]

    rpi, emb = _twice(run)
    want = R.reference_points_input(ref, vr)
    assert torch.equal(rpi.view(torch.int32), want.contiguous().view(torch.int32)), "reference_points_input is not the fp32 product"
    assert bool((emb[:, 512:].contiguous().view(torch.int16) == SENT_BF).all()), "columns past 512 must stay untouched"
    e64 = R.query_sine_embed(want[:, :, 0, :].to(F64), dtype=F64).view(B * nq, 512)
    worst = float(((emb[:, :512].to(F64) - e64).abs() / (2.0 ** -8 * e64.abs() + 2.0 ** -18)).max())
    print(f"query_sine nq={nq} L={L}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


def test_query_sine_reproduces_the_reference_fixture():
    from anyedit_amd import ops
    z = load_golden("gdino_dec_geom")
    boxes, ref = T(z["boxes"]), T(z["sineembed"])
    B, nq = boxes.shape[:2]
    _, emb = ops.gdino_query_sine(boxes.to(DEV), torch.ones(B, 1, 2, device=DEV))
    err = (emb.float().cpu().view(B, nq, 512) - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 2.0 ** -18).all())


# ------------------------------------------------------------------------------------------------------------------ box refinement
@pytest.mark.parametrize("M", [1, 5, 1800])
@pytest.mark.parametrize("logit", [False, True])
def test_box_refine_vs_fp32_formula(M, logit):
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(M + int(logit))
    h = torch.randn(M, 256, generator=gen)
    w3 = torch.randn(4, 256, generator=gen) / 16
    b3 = torch.randn(4, generator=gen)
    if logit:
        ref = 3 * torch.randn(M, 4, generator=gen)
        ref[::3] = INF                   # padded / invalid proposals
    else:
        ref = torch.rand(M, 4, generator=gen)
        ref[0] = torch.tensor([0.0, 1.0, 0.5, 0.0])
        ref[M - 1, 3] = 1.0
    ldh = 256 + 12
    hw = torch.full((M, ldh), float("nan"))
    hw[:, :256] = h
    dh = hw.to(DEV)[:, :256]
    dw, db, dr = w3.to(DEV), b3.to(DEV), ref.to(DEV)

    def run():
        gb, gu = Guarded((M, 4), torch.float32), Guarded((M, 4), torch.float32)
        ops.gdino_box_refine(dh, dw, db, dr, ref_is_logit=logit, boxes=gb.t, unsigmoid=gu.t)
        return [gb, gu]

    boxes, u = _twice(run)
    sref, uref = R.box_refine(h, w3, b3, ref, ref_is_logit=logit)
    assert not torch.isnan(boxes).any() and not torch.isnan(u).any()
    inf_rows = torch.isposinf(uref)
    assert torch.equal(torch.isposinf(u), inf_rows) and bool((boxes[inf_rows] == 1.0).all())
    if logit:
        assert bool(inf_rows[::3].all())
    fin = ~inf_rows
    bound = 2.0 ** -15 * ((h.abs().double() @ w3.abs().double().t()) + b3.abs().double()) + 2.0 ** -20 * (1 + torch.where(fin, uref, torch.zeros_like(uref)).abs().double())
    wu = float(((u.double() - uref.double()).abs()[fin] / bound[fin]).max()) if fin.any() else 0.0      # M = 1 with ref_is_logit: the one row is +inf
    ws = float(((boxes.double() - sref.double()).abs()[fin] / (bound[fin] / 4 + 2.0 ** -22)).max()) if fin.any() else 0.0
    print(f"box_refine M={M} ref_is_logit={logit}: worst |err| / bound  u {wu:.3f}  sigmoid {ws:.3f}")
    assert wu <= 1.0 and ws <= 1.0


def test_box_refine_without_u_writes_boxes_only():
    from anyedit_amd import ops
    h = torch.randn(6, 256, device=DEV)
    w3, b3, ref = torch.randn(4, 256, device=DEV) / 16, torch.randn(4, device=DEV), torch.rand(6, 4, device=DEV)
    a = ops.gdino_box_refine(h, w3, b3, ref)
    b, u = ops.gdino_box_refine(h, w3, b3, ref, want_unsigmoid=True)
    assert torch.equal(a, b) and torch.equal(u.sigmoid().isfinite(), torch.ones_like(u, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------------------------ the reference's names
def test_utils_modules_run_on_the_kernels():
    """groundingdino/utils.py: MLP (fp32, fused refine), ContrastiveEmbed (+ rowmax), gen_encoder_output_proposals, gen_sineembed_for_position and
    inverse_sigmoid under the reference's names and signatures, against the restatement with the bounds of the kernel tests."""
    from anyedit_amd.groundingdino import utils as U
    gen = torch.Generator().manual_seed(5)
    z = load_golden("gdino_dec_geom")
    # proposals: the reference's two outputs
    mask, shapes = T(z["padding_mask"]), T(z["spatial_shapes"])
    mem = torch.randn(mask.shape[0], mask.shape[1], 8, generator=gen)
    om, prop, keep = U.gen_encoder_output_proposals(mem.to(DEV), mask.to(DEV), shapes, want_keep=True)
    kept = T(z["memory_kept"])
    assert torch.equal(keep.bool().cpu(), kept) and torch.equal(om.cpu(), mem * kept[..., None]) and torch.equal(torch.isposinf(prop.cpu()), torch.isposinf(T(z["proposals"])))
    with pytest.raises(NotImplementedError, match="learnedwh"):
        U.gen_encoder_output_proposals(mem.to(DEV), mask.to(DEV), shapes, learnedwh=torch.zeros(2))
    # sine embedding, [nq, bs, 4] in, [nq, bs, 512] out
    boxes, sine = T(z["boxes"]), T(z["sineembed"])
    emb = U.gen_sineembed_for_position(boxes.to(DEV)).cpu()
    assert emb.shape == sine.shape and emb.dtype == torch.float32 and bool(((emb - sine).abs() <= 2.0 ** -8 * sine.abs() + 2.0 ** -18).all())
    with pytest.raises(NotImplementedError, match="2-d"):
        U.gen_sineembed_for_position(boxes[..., :2].to(DEV))
    # contrastive head and its row maximum
    x, y, m = T(z["ce_x"]), T(z["ce_y"]), T(z["ce_mask"])
    ce = U.ContrastiveEmbed(max_text_len=16)
    td = {"encoded_text": y.to(DEV), "text_token_mask": m.to(DEV)}
    lg, rm = ce(x.to(DEV), td), ce.rowmax(x.to(DEV), td)
    assert lg.shape == (2, 5, 16) and torch.equal(torch.isneginf(lg.cpu()), torch.isneginf(T(z["ce_out"]))) and torch.equal(rm, lg.max(-1)[0])
    # box MLP: forward, and the fused update against the fp32 formula
    mlp = U.MLP(256, 256, 4, 3)
    assert sorted(mlp.state_dict()) == sorted(f"layers.{i}.{n}" for i in range(3) for n in ("weight", "bias"))
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.06 if p.dim() == 2 else 0.1))
    hs = torch.randn(2, 7, 256, generator=gen).to(BF)
    ref = torch.rand(2, 7, 4, generator=gen)
    lin = torch.nn.functional.linear
    L0, L1, L2 = mlp.layers
    hid = lin(lin(hs.float(), L0.weight, L0.bias).relu(), L1.weight, L1.bias).relu()
    delta = lin(hid, L2.weight, L2.bias)
    dmlp = U.MLP(256, 256, 4, 3).to(DEV)
    dmlp.load_state_dict(mlp.state_dict())
    with torch.no_grad():
        got_delta = dmlp(hs.to(DEV)).cpu()
        got_hid = dmlp.hidden(hs.to(DEV)).cpu()
        boxes_d, u_d = dmlp.refine(hs.to(DEV), ref.to(DEV), want_unsigmoid=True)
    # three fp32 layers of 256 terms: every sum within 2^-15 of its sum of magnitudes (the contrastive bound), carried through two more layers
    tol = 3 * 2.0 ** -15 * float((hid.abs() @ L2.weight.abs().t() + L2.bias.abs()).max()) + 1e-5
    assert float((got_delta - delta).abs().max()) <= tol
    sref, uref = R.box_refine(got_hid.view(-1, 256), L2.weight.detach(), L2.bias.detach(), ref.view(-1, 4))
    bound = 2.0 ** -15 * ((got_hid.view(-1, 256).abs().double() @ L2.weight.detach().abs().double().t()) + L2.bias.detach().abs().double()) + 2.0 ** -20 * (1 + uref.abs().double())
    assert bool(((u_d.cpu().view(-1, 4).double() - uref.double()).abs() <= bound).all())
    assert bool(((boxes_d.cpu().view(-1, 4).double() - sref.double()).abs() <= bound / 4 + 2.0 ** -22).all())
    assert boxes_d.shape == (2, 7, 4)
    with pytest.raises(ValueError, match="256 -> 4"):
        U.MLP(512, 256, 256, 2).to(DEV).refine(torch.zeros(1, 512, device=DEV), torch.zeros(1, 4, device=DEV))
    xs = torch.tensor([0.0, 1.0, 0.5, 1e-3, 5e-4, -0.2, 1.3, 0.25])
    assert torch.equal(U.inverse_sigmoid(xs), R.inverse_sigmoid(xs))


def test_query_selection_on_the_kernels_matches_its_torch_form():
    """transformer.py:291-301 at a small size: rowmax + top-k against matmul + masked_fill + max + stable sort on the same bf16 operands.  Rows of
    zeros (the masked rows of query selection) tie exactly and must come out by ascending index."""
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(9)
    B, N, Tn, C, k = 2, 700, 12, 256, 90
    x = torch.randn(B, N, C, generator=gen).to(BF)
    x[:, torch.randperm(N, generator=gen)[:650]] = x[:, :1]          # 650 identical rows per sample: more ties than k
    y = torch.randn(B, Tn, C, generator=gen).to(BF)
    m = torch.ones(B, Tn, dtype=torch.bool)
    m[1, 7:] = False
    _, rm = ops.contrastive(x.to(DEV), y.to(DEV), m.to(DEV), max_text_len=256, want_logits=False, want_rowmax=True)
    idx = ops.topk_rows(rm, k).cpu()
    assert torch.equal(idx, R.stable_topk(rm.cpu(), k).to(torch.int32)), "selection is not the stable sort of the kernel's own scores"
    tie = rm.cpu()[:, 0]
    tied_sel = [idx[b][rm.cpu()[b, idx[b].long()] == tie[b]] for b in range(B)]
    assert all(len(t) > 1 and bool((t[1:] > t[:-1]).all()) for t in tied_sel), "tied rows must be selected by ascending index"
    ref = R.contrastive(x.to(F64), y.to(F64), m, 256).max(-1)[0]
    mag = (x.to(F64).abs() @ y.to(F64).abs().transpose(1, 2)).max(-1)[0]
    assert bool(((rm.cpu().to(F64) - ref).abs() <= 2.0 ** -15 * mag).all())


def test_prediction_heads_restate_the_model_class():
    """groundingdino.py:317-335 on given decoder outputs: boxes against the fp32 formula under the box bound carried through the MLP's fp32 layers,
    logits against float64 on the bf16 operands under the contrastive bound; a shared box head, as the SwinB config wires it."""
    from anyedit_amd.groundingdino import utils as U
    from anyedit_amd.groundingdino.transformer import prediction_heads
    gen = torch.Generator().manual_seed(21)
    B, nq, Tn, nl = 2, 20, 12, 2
    mlp = U.MLP(256, 256, 4, 3)
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.06 if p.dim() == 2 else 0.1))
    dmlp = U.MLP(256, 256, 4, 3).to(DEV)
    dmlp.load_state_dict(mlp.state_dict())
    hs = [torch.randn(B, nq, 256, generator=gen).to(BF).float() for _ in range(nl)]
    refs = [torch.rand(B, nq, 4, generator=gen) for _ in range(nl + 1)]
    y = torch.randn(B, Tn, 256, generator=gen).to(BF).float()
    m = torch.ones(B, Tn, dtype=torch.bool)
    m[1, 7:] = False
    td = {"encoded_text": y.to(DEV), "text_token_mask": m.to(DEV)}
    with torch.no_grad():
        out = prediction_heads([h.to(DEV) for h in hs], [r.to(DEV) for r in refs], [dmlp] * nl, [U.ContrastiveEmbed(256)] * nl, td, aux=True)
    assert set(out) == {"pred_logits", "pred_boxes", "aux_outputs"} and len(out["aux_outputs"]) == nl - 1
    lin = torch.nn.functional.linear
    L0, L1, L2 = mlp.layers
    for l, got in ((nl - 1, out), (0, out["aux_outputs"][0])):
        with torch.no_grad():
            hid = lin(lin(hs[l], L0.weight, L0.bias).relu(), L1.weight, L1.bias).relu()
            sref, _ = R.box_refine(hid.view(-1, 256), L2.weight, L2.bias, refs[l].view(-1, 4))
            # two fp32 layers ahead of the fused one: their sums are within 2^-15 of their magnitudes, and the last layer carries that on
            slack = 3 * 2.0 ** -15 * float((hid.abs() @ L2.weight.abs().t() + L2.bias.abs()).max()) + 1e-5
        assert got["pred_boxes"].shape == (B, nq, 4) and float((got["pred_boxes"].cpu().view(-1, 4) - sref).abs().max()) <= slack / 4 + 2.0 ** -22
        ref = R.contrastive(hs[l].to(F64), y.to(F64), m, 256)
        mag = R.contrastive(hs[l].to(F64).abs(), y.to(F64).abs(), m, 256)
        lg = got["pred_logits"].cpu()
        fin = torch.isfinite(ref)
        assert lg.shape == (B, nq, 256) and torch.equal(torch.isneginf(lg), ~fin)
        assert bool(((lg.to(F64) - ref)[fin].abs() <= 2.0 ** -15 * mag[fin] + 1e-30).all())
    with pytest.raises(ValueError, match="references"):
        prediction_heads([hs[0].to(DEV)], [refs[0].to(DEV)], [dmlp], [U.ContrastiveEmbed(256)], td)


# ------------------------------------------------------------------------------------------------------------------ existing attention, new sizes
@pytest.mark.parametrize("Nk,masked", [(900, False), (7, True), (256, True)])
def test_attention_at_the_decoders_shapes(Nk, masked):
    """ops.attention (existing code) at the decoder's sizes: head dim 32, 8 heads, 900 queries; self-attention over the 900 queries without a mask,
    text cross-attention over 7 / 256 keys under a key mask (0 = masked, the kernel's sense).  Attention rule of tests/test_hip_gdino_encoder.py:
    every element within 2^-8 |ref| + 2^-8 (P @ |V|) + 1e-30 of float64 on the same bf16 inputs."""
    from anyedit_amd import ops
    B, H, D, Nq = 2, 8, 32, 900
    C = H * D
    gen = torch.Generator().manual_seed(Nk)
    q = torch.randn(B, Nq, C, generator=gen).to(BF)
    k = torch.randn(B, Nk, C, generator=gen).to(BF)
    v = torch.randn(B, Nk, C, generator=gen).to(BF)
    live = torch.ones(B, Nk, dtype=torch.bool)
    if masked:
        live = torch.rand(B, Nk, generator=gen) < 0.5
        live[0, Nk // 2] = True
        live[1] = False
        live[1, Nk - 1] = True                      # one sample with a single used token, the last one
    scale = D ** -0.5
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), B, H, Nq, Nk, D, scale, (Nq * C, D, C), (Nk * C, D, C), (Nk * C, D, C),
                        key_mask=live.to(torch.uint8).to(DEV) if masked else None)
    torch.cuda.synchronize()
    sp = lambda t, n: t.to(F64).view(B, n, H, D).permute(0, 2, 1, 3)
    S = scale * sp(q, Nq) @ sp(k, Nk).transpose(-1, -2)
    S = S.masked_fill(~live[:, None, None, :], float("-inf"))
    P = S.softmax(-1)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, Nq, C)
    ref, pav = back(P @ sp(v, Nk)), back(P @ sp(v, Nk).abs())
    got = out.cpu().to(F64)
    assert torch.isfinite(got).all()
    worst = float(((got - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -8 * pav + 1e-30)).max())
    print(f"attention D=32 Nq={Nq} Nk={Nk} key_mask={masked}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ the tower
# Tower rule (the project's): rel-L2 of the HIP path <= 1.5 x the control's, both against the same fp32 reference; the control is the restatement
# rounding to bf16 wherever the HIP path stores bf16.  The tensors named in NO_BF16_STORE have no bf16 store in front of them: the control is then
# bit-equal to the reference and 1.5 x 0 admits no fp32 rounding at all, so they (and only they) are held to 2^-19 instead, the proposals kernel's
# own bound (one rounding of the quotient, a few ulps of logf, contracted by the sigmoid).  Reasoned, not measured.
FP32_BOUND = 2.0 ** -19
NO_BF16_STORE = {"standard": ("init_box_proposal",), "no": ("init_box_proposal", "dec.0.reference_points")}


def _rel_fin(a, b):
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin)
    a, b = a.double()[fin], b.double()[fin]
    return float((a - b).norm() / (b.norm() + 1e-30))


def _judge(name, hip, ctl, ref, report, fp32_only=False):
    e_hip, e_ctl = _rel_fin(hip.float().cpu(), ref), _rel_fin(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}" + ("  (no bf16 store: held to 2^-19)" if fp32_only else ""))
    return e_hip <= (FP32_BOUND if fp32_only else 1.5 * e_ctl)


_CACHE = {}


def _tower(two_stage):
    if two_stage not in _CACHE:
        _CACHE[two_stage] = R.tower_module(two_stage, DEV)
    return _CACHE[two_stage]


def _io():
    if "io" not in _CACHE:
        _CACHE["io"], _CACHE["sd"] = R.tower_io(), R.tower_weights()
    return _CACHE["io"], _CACHE["sd"]


def _run_tower(two_stage, forced, sample=None):
    """One forward of the HIP tower on the golden's inputs (optionally one sample of them) + prediction_heads; every tensor the golden stores."""
    from anyedit_amd.groundingdino.transformer import prediction_heads
    io, _ = _io()
    m = _tower(two_stage)
    sl = (lambda t: t) if sample is None else (lambda t: t[sample:sample + 1])
    srcs, masks, poss, text, tm = R.tower_inputs(io)
    d = lambda t: sl(t).to(DEV)
    td = {"encoded_text": d(text), "text_token_mask": d(tm)}
    taps = {}

    def tap(l, x, ref, sine):
        taps[f"dec.{l}.output"], taps[f"dec.{l}.reference_points"] = x.float().clone(), ref.clone()
        taps[f"dec.{l}.query_sine_embed"] = sine.float().view(x.shape[0], x.shape[1], 512).clone()
    m.decoder.tap = tap
    idx = d(io["topk_proposals"]) if forced and two_stage == "standard" else None
    try:
        hs, refs, hs_enc, ref_enc, ibp = m([d(s) for s in srcs], [d(k) for k in masks], None, [d(p) for p in poss], None, None, td, topk_proposals=idx)
    finally:
        m.decoder.tap = None
    out = dict(taps, hs=torch.stack(hs), references=torch.stack(refs), init_box_proposal=ibp)
    if two_stage == "standard":
        out.update(hs_enc=hs_enc, ref_enc=ref_enc, topk_logits=m.last_topk_logits)
        if not forced:
            out["selected"] = m.last_topk_proposals
    heads = prediction_heads(hs, refs, m.decoder.bbox_embed, m.decoder.class_embed, td, aux=True)
    for l, h in enumerate(heads["aux_outputs"] + [heads]):
        out[f"pred_boxes.{l}"], out[f"pred_logits.{l}"] = h["pred_boxes"], h["pred_logits"]
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _control(two_stage):
    key = "ctl." + two_stage
    if key not in _CACHE:
        io, sd = _io()
        srcs, masks, _, text, tm = R.tower_inputs(io)
        _CACHE[key] = R.transformer_forward(sd, R.GEOM, srcs, masks, text, tm, two_stage=two_stage, store=R.round_bf16,
                                            topk_proposals=io["topk_proposals"] if two_stage == "standard" else None)
    return _CACHE[key]


@pytest.mark.parametrize("two_stage", ["standard", "no"])
def test_tower_reproduces_the_golden_with_forced_selection(two_stage):
    io, _ = _io()
    pre = "" if two_stage == "standard" else "no."
    got, ctl = _run_tower(two_stage, forced=True), _control(two_stage)
    report, ok, n = [], True, 0
    for k, hip in got.items():
        if k == "references" and two_stage == "no":          # references[0] is the tensor named above; the rest follows the rule
            ok &= _judge("references[0]", hip[0], ctl[k][0], io[pre + k][0], report, fp32_only=True)
            ok &= _judge("references[1:]", hip[1:], ctl[k][1:], io[pre + k][1:], report)
        else:
            ok &= _judge(k, hip, ctl[k], io[pre + k], report, fp32_only=k in NO_BF16_STORE[two_stage])
        n += 1
    print("\n".join(report))
    assert n == (16 if two_stage == "standard" else 13), n      # every stored float tensor (the indices are forced)
    assert ok, "\n".join(report)


def test_tower_unforced_selection():
    io, _ = _io()
    nq = R.GEOM["num_queries"]
    forced, free, ctl = _run_tower("standard", True), _run_tower("standard", False), _control("standard")
    ref_s = io["topk_logits"]
    report = []
    assert _judge("topk_logits", free["topk_logits"], ctl["topk_logits"], ref_s, report), report
    e = float((ctl["topk_logits"] - ref_s).abs().max())          # the control's largest score deviation
    sel = free.pop("selected")
    assert torch.equal(sel, R.stable_topk(free["topk_logits"], nq)), "the selection is not the stable sort of the tower's own scores"
    s_k = torch.sort(ref_s, 1, descending=True)[0][:, nq - 1]
    for b in range(sel.shape[0]):
        chosen = torch.zeros(ref_s.shape[1], dtype=torch.bool)
        chosen[sel[b]] = True
        assert bool((ref_s[b][sel[b]] >= s_k[b] - 2 * e).all()), "a selected row scores below the k-th reference score by more than 2e"
        assert bool(chosen[ref_s[b] > s_k[b] + 2 * e].all()), "a row above the k-th reference score by more than 2e is not selected"
    same = torch.equal(sel, io["topk_proposals"])
    print(f"unforced selection: e = {e:.3e}, indices equal to the reference's: {same}")
    if same:
        for k in forced:
            assert torch.equal(forced[k], free[k]), k
    else:
        hit = sel == io["topk_proposals"]                        # slot by slot, only where the index matches; the decoder mixes the slots
        for k in ("init_box_proposal",):
            assert torch.equal(forced[k][hit], free[k][hit]), k
        for k in ("hs_enc", "ref_enc"):
            assert torch.equal(forced[k][0][hit], free[k][0][hit]), k


def test_tower_batch_independence():
    both, one = _run_tower("standard", True), _run_tower("standard", True, sample=0)
    for k, v in one.items():
        full = both[k]
        part = full[:, :1] if k in ("hs", "references", "hs_enc", "ref_enc") else full[:1]
        assert torch.equal(part.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), f"{k}: sample 0 alone differs from sample 0 of the batch"


def test_tower_graph_capture_replays_the_eager_result():
    io, _ = _io()
    m = _tower("standard")
    srcs, masks, poss, text, tm = R.tower_inputs(io)
    d = lambda t: t.to(DEV)
    S, K, P, idx = [d(s) for s in srcs], [d(k) for k in masks], [d(p) for p in poss], d(io["topk_proposals"])
    text_d, tm_d = d(text), d(tm)

    def fwd():
        hs, refs, hs_enc, ref_enc, ibp = m(S, K, None, P, None, None, {"encoded_text": text_d, "text_token_mask": tm_d})
        return torch.stack(hs), torch.stack(refs), hs_enc, ref_enc, ibp

    eager = [t.clone() for t in fwd()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd()                                   # warm the allocator and the caches on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = fwd()
        for t in outs:
            t.zero_()
        g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8)), "the replay differs from the eager forward"


def test_decoder_at_production_width():
    """TransformerDecoder.forward at 6 layers, dim_feedforward 2048, 900 queries, four levels of 3 060 tokens, on given tgt / refpoints, against the
    restatement under the tower rule."""
    import gdino_enc_ref as E
    from anyedit_amd.groundingdino.transformer import DeformableTransformerDecoderLayer, TransformerDecoder
    from anyedit_amd.groundingdino.utils import MLP
    levels, nq, Nt, B, nl = [(48, 48), (24, 24), (12, 12), (6, 6)], 900, 16, 1, 6
    N = sum(h * w for h, w in levels)
    gen = torch.Generator().manual_seed(66)
    torch.manual_seed(66)
    dec = TransformerDecoder(DeformableTransformerDecoderLayer(256, 2048, 0.0, "relu", 4, 8, 4, use_text_cross_attention=True), nl, torch.nn.LayerNorm(256),
                             return_intermediate=True, d_model=256, query_dim=4, num_feature_levels=4)
    dec.bbox_embed = torch.nn.ModuleList([MLP(256, 256, 4, 3)] * nl)
    for mod in dec.modules():
        if hasattr(mod, "_reset_parameters") and type(mod).__name__ == "MultiScaleDeformableAttention":
            mod._reset_parameters()
    sd = E.draw_weights(dec.state_dict(), gen)
    for k in list(sd):
        if k.startswith("bbox_embed."):         # one shared head, listed under every layer's index
            sd[k] = sd["bbox_embed.0." + k.split(".", 2)[2]]
    for k in list(sd):
        if k.startswith("bbox_embed.") and k.endswith("layers.2.weight"):
            sd[k] = R.round_bf16(sd["bbox_embed.0.layers.2.weight"] * 0.1) if k != "bbox_embed.0.layers.2.weight" else sd[k]
    sd["bbox_embed.0.layers.2.weight"] = sd["bbox_embed.1.layers.2.weight"]      # box deltas of a trained head are small: the boxes stay inside the image
    dec.load_state_dict(sd)
    dec = dec.eval().requires_grad_(False).to(DEV)
    tgt = torch.randn(B, nq, 256, generator=gen)
    unsig = R.inverse_sigmoid(torch.cat((0.1 + 0.8 * torch.rand(B, nq, 2, generator=gen), 0.05 + 0.3 * torch.rand(B, nq, 2, generator=gen)), -1))
    mem = torch.randn(B, N, 256, generator=gen).to(BF).float()
    text = torch.randn(B, Nt, 256, generator=gen)
    pad = torch.zeros(B, Nt, dtype=torch.bool)
    pad[:, 11:] = True
    kpm = torch.zeros(B, N, dtype=torch.bool)
    vr = torch.ones(B, 4, 2)
    shapes = torch.tensor(levels)
    starts = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    hs, refs = dec(tgt.transpose(0, 1).to(DEV), mem.transpose(0, 1).to(DEV), memory_key_padding_mask=kpm.to(DEV), refpoints_unsigmoid=unsig.transpose(0, 1).to(DEV),
                   level_start_index=starts.to(DEV), spatial_shapes=shapes, valid_ratios=vr.to(DEV), memory_text=text.to(DEV), text_attention_mask=pad.to(DEV))
    torch.cuda.synchronize()
    cfg = dict(num_decoder_layers=nl, nhead=8, points=4)
    runs = []
    for store in (None, R.round_bf16):
        c = E._Ctx(sd, store)
        runs.append(R.decoder_forward(c, "", cfg, tgt, unsig, mem, levels, vr, kpm, c.st(text), pad, {}))
    report, ok = [], True
    for l in range(nl):
        ok &= _judge(f"hs[{l}]", hs[l], runs[1][0][l], runs[0][0][l], report)
        ok &= _judge(f"references[{l + 1}]", refs[l + 1], runs[1][1][l + 1], runs[0][1][l + 1], report)
    print("\n".join(report))
    assert ok, "\n".join(report)
