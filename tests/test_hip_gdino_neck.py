"""GPU tests of GroundingDINO's neck and grounded-box filter (anyedit_amd/csrc/gdino_neck.hip): every kernel writes into sentinel-filled buffers
between guard bands, is launched twice and must give bit-identical outputs.  Every case runs once.

Bounds, each from the arithmetic and not from what the kernels give:
  level geometry   mask_flatten exactly the integer nearest resize; valid_ratios bit-equal to the fp32 quotient count / size (so the two counts
                   are exact); the embedding within 2^-8 |ref| + 2^-17 of float64 (tests/gdino_neck_ref.py): one bf16 rounding, at most eight
                   fp32 roundings of an argument <= 2 pi (8 * 2^-24 * 2 pi = 3e-6) and the device sin / cos.  A prefix count that is off by one
                   moves the argument of the first channel pair by 2 pi / e_last >= 2 pi / 300 here, three orders above the bound: the counts
                   are pinned through the embedding.
  neck GroupNorm   every element within tests/norm_ref.py's two-pass bound (`forward(..., onepass=False)`, `check_elements`); the rows of the
                   output buffer in front of and behind the level's slice stay untouched.
  grounding        count, indices, order and token bit sets exactly those of the CPU statement of tools/tool.py:125-141; scores within 2^-22 of
                   torch's fp32 sigmoid on the CPU (two ulps below 1); boxes bit-equal; the rows behind `count` are index -1 and zeros.  The
                   logits are drawn so that no sigmoid lies within 1e-5 of a threshold and no score within 1e-4 of a multiple of 0.01 (the
                   4-character score of a phrase is then the same on both sides); both conditions are asserted on the CPU reference first.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, T  # noqa: E402
import gdino_neck_ref as R  # noqa: E402
import norm_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
GUARD = 4096
SENT_BYTE = 0xFF


class Guarded:
    """A tensor of `shape` / `dtype` inside a byte buffer filled with 0xFF, with GUARD bytes of the same before and after it."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((n + 2 * GUARD,), SENT_BYTE, dtype=torch.uint8, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(*shape)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT_BYTE).all()) and bool((self.buf[-GUARD:] == SENT_BYTE).all())


def _twice(fn):
    runs = []
    for _ in range(2):
        outs = fn()
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs), "wrote outside its outputs"
        runs.append([o.t.clone().cpu() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), "two launches differ"
    return runs[0]


# ------------------------------------------------------------------------------------------------------------------ level geometry
def _holes_mask(B, H, W, seed, col, row):
    """random holes, one fully padded column band and one fully padded row band; sample 0 stays unpadded"""
    gen = torch.Generator().manual_seed(seed)
    m = torch.rand(B, H, W, generator=gen) < 0.3
    m[:, :, col[0]:col[1]] = True
    m[:, row[0]:row[1], :] = True
    m[0] = False
    return m


def _geom_cases():
    g = load_golden("gdino_dec_geom")
    flat = T(g["padding_mask"])                                                      # [3, 32]: levels (1,1) (3,5) (4,3) (2,2)
    shapes = [tuple(int(v) for v in s) for s in g["spatial_shapes"]]
    assert shapes == [(1, 1), (3, 5), (4, 3), (2, 2)]
    lvl35 = flat[:, 1:16].view(3, 3, 5)
    cases = {"four_levels": (lvl35.repeat_interleave(4, 1).repeat_interleave(4, 2), shapes, True, (20.0, 20.0))}
    st = 0
    for i, (h, w) in enumerate(shapes):                                              # each fixture mask as its own level (identity resize)
        cases[f"fixture_level{i}"] = (flat[:, st:st + h * w].view(3, h, w), [(h, w)], i % 2 == 0, (20.0, 20.0))
        st += h * w
    cases["holes_70x130"] = (_holes_mask(2, 140, 260, 1, (100, 104), (60, 64)), [(70, 130)], True, (20.0, 20.0))
    cases["holes_wide_3x300"] = (_holes_mask(2, 7, 650, 2, (300, 306), (3, 5)), [(3, 300), (2, 5)], False, (10000.0, 20.0))
    cases["w1"] = (_holes_mask(2, 11, 1, 3, (0, 0), (4, 6)), [(11, 1), (6, 1)], True, (20.0, 10000.0))
    cases["no_mask"] = (None, [(6, 9), (3, 5)], True, (20.0, 20.0))
    return cases


GEOM = None


@pytest.mark.parametrize("name", ["four_levels", "fixture_level0", "fixture_level1", "fixture_level2", "fixture_level3", "holes_70x130", "holes_wide_3x300",
                                  "w1", "no_mask"])
def test_level_geometry(name):
    from anyedit_amd import ops
    global GEOM
    if GEOM is None:
        GEOM = _geom_cases()
    mask, shapes, with_le, (tH, tW) = GEOM[name]
    L = len(shapes)
    B = 2 if mask is None else mask.shape[0]
    N = sum(h * w for h, w in shapes)
    le = (torch.randn(L, 256, generator=torch.Generator().manual_seed(7)) if with_le else None)
    dm = None if mask is None else mask.to(DEV)
    dle = None if le is None else le.to(DEV)

    def run():
        gm, gp, gv = Guarded((B, N), torch.bool), Guarded((B, N, 256), BF), Guarded((B, L, 2), torch.float32)
        ops.gdino_level_geometry(dm, shapes, B, tH, tW, dle, device=DEV, mask_flatten=gm.t, pos_flatten=gp.t, valid_ratios=gv.t)
        return [gm, gp, gv]

    mf, pf, vr = _twice(run)
    ref_mask = torch.zeros(B, shapes[0][0], shapes[0][1], dtype=torch.bool) if mask is None else mask
    rm, rp, rv, _ = R.level_geometry(ref_mask, shapes, tH, tW, le, F64)
    assert torch.equal(mf.view(torch.uint8), rm.view(torch.uint8)), "mask_flatten"
    assert torch.equal(vr.view(torch.int32), rv.view(torch.int32)), f"valid_ratios {vr} against {rv}"
    if name.startswith("holes"):
        lm = R.level_mask(ref_mask, *shapes[0])
        assert bool(lm[1].all(0).any()) and bool(lm[1].all(1).any()) and not bool(lm[1].all()), "the case must hold a fully padded column and row"
    err = (pf.to(F64) - rp).abs()
    bound = 2.0 ** -8 * rp.abs() + 2.0 ** -17
    worst = float((err / bound).max())
    print(f"level geometry {name}: worst error / bound {worst:.3f}; worst |error| before the bf16 allowance {float((err - 2.0 ** -8 * rp.abs()).max()):.3g}")
    assert worst <= 1.0


def test_position_embedding_module_matches_fixture():
    """PositionEmbeddingSineHW on the kernel (L = 1, no level embedding) against the reference's own output, NCHW fp32 as the reference returns it."""
    from anyedit_amd.groundingdino.misc import NestedTensor
    from anyedit_amd.groundingdino.position_encoding import PositionEmbeddingSineHW
    g = load_golden("gdino_neck")
    pe = PositionEmbeddingSineHW(128, temperatureH=20, temperatureW=20, normalize=True)
    for l in range(4):
        lm = T(g[f"lmask.{l}"]).to(DEV)
        ref = T(g[f"pos.{l}"]).to(F64)
        out = pe(NestedTensor(torch.zeros(3, 1, *lm.shape[1:], device=DEV), lm))
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape)
        assert bool(((out.cpu().to(F64) - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -17 + 2.0 ** -22).all())   # + the fixture's own fp32 arithmetic


# ------------------------------------------------------------------------------------------------------------------ neck GroupNorm
@pytest.mark.parametrize("hw", [1, 2, 63, 64, 65, 169, 10000])
def test_neck_groupnorm(hw):
    from anyedit_amd import ops
    B, C, G, eps = 2, 256, 32, 1e-5
    gen = torch.Generator().manual_seed(100 + hw)
    x = NR.make_x(gen, B, hw, C, G)                                                   # bf16 values: exact in fp32
    gamma, beta = NR.make_affine(gen, C)
    ref = NR.forward(x, gamma, beta, G, eps, 0, onepass=False)
    dx, dg, db = x.float().view(B * hw, C).to(DEV), gamma.to(DEV), beta.to(DEV)
    off, N = 3, hw + 8                                                                # a batch stride wider than the level

    def run():
        go = Guarded((B, N, C), BF)
        ops.gdino_neck_groupnorm(dx, dg, db, B, hw, eps, out=go.t, row_offset=off)
        return [go]

    (out,) = _twice(run)
    rest = torch.cat([out[:, :off], out[:, off + hw:]], 1).contiguous().view(torch.int16)
    assert bool((rest == -1).all()), "the neighbouring rows of the concatenated buffer must stay untouched"
    ratio = NR.check_elements(out[:, off:off + hw], ref["y"], ref["bnd"], f"neck groupnorm hw={hw}")
    print(f"neck groupnorm hw={hw}: worst error / two-pass bound {ratio:.3f}")


def test_neck_groupnorm_on_projection_fixture():
    """The two input_proj levels of the fixture (torch's Conv2d + GroupNorm in fp32) through ops.gemm / ops.conv3x3 (fp32 out) and the kernel:
    rel-L2 below 2^-8 (one bf16 rounding of the activations entering the projection is already in the fixture's x; one of the result)."""
    from anyedit_amd import ops
    from conftest import rel_l2
    g = {k: T(v) for k, v in load_golden("gdino_neck").items()}
    B, Cin, H, W = g["proj1.x"].shape
    rows = lambda x: x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()
    x1 = rows(g["proj1.x"]).to(DEV, BF)
    u = ops.gemm(x1, ops.pack_linear(g["proj1.w"].view(256, Cin).to(DEV)), g["proj1.b"].to(DEV), out_f32=True)
    y = ops.gdino_neck_groupnorm(u, g["proj1.g"].to(DEV), g["proj1.e"].to(DEV), B, H * W)
    e1 = rel_l2(y.float().cpu(), rows(g["proj1.y"]).view(B, H * W, 256))
    x2 = rows(g["proj2.x"]).to(DEV, BF)
    u, h2, w2 = ops.conv3x3(x2, ops.pack_conv3x3(g["proj2.w"].to(DEV)), g["proj2.b"].to(DEV), B, H, W, stride=2, out_f32=True)
    assert (h2, w2) == tuple(g["proj2.y"].shape[-2:])
    y = ops.gdino_neck_groupnorm(u, g["proj2.g"].to(DEV), g["proj2.e"].to(DEV), B, h2 * w2)
    e2 = rel_l2(y.float().cpu(), rows(g["proj2.y"]).view(B, h2 * w2, 256))
    print(f"input_proj against the fixture: 1x1 rel-L2 {e1:.3g}, 3x3 stride 2 rel-L2 {e2:.3g}")
    assert e1 <= 2.0 ** -8 and e2 <= 2.0 ** -8


# ------------------------------------------------------------------------------------------------------------------ grounding filter
BOX_T, TEXT_T = 0.3, 0.25


def _logit(p):
    return float(np.log(p / (1 - p)))


def _ground_inputs(nq, Tn, seed):
    """B = 3: image 0 random with unused (-inf) columns and some rows all -inf, image 1 keeps nothing, image 2 keeps everything"""
    gen = torch.Generator().manual_seed(seed)
    lg = torch.randn(3, nq, Tn, generator=gen) * 2.0 - 1.5
    used = max(3, Tn - 11)
    lg[0, :, used:] = -float("inf")
    lg[0, torch.arange(nq) % 5 == 2] = -float("inf")
    lg[1] = lg[1].clamp(max=_logit(BOX_T) - 0.5)
    lg[1, nq // 2] = -float("inf")
    lg[2, :, 1] = lg[2, :, 1].clamp(min=_logit(BOX_T) + 0.5)
    for _ in range(50):                                                               # move the values off the three decision edges
        p = lg.sigmoid()
        near = ((p - BOX_T).abs() < 2e-5) | ((p - TEXT_T).abs() < 2e-5)
        s = p.max(-1)[0]
        frac = (s * 100 - (s * 100).round()).abs() / 100
        bad = (frac < 2e-4) & (s > 0)
        if not bool(near.any()) and not bool(bad.any()):
            break
        lg = torch.where(near, lg + 0.01, lg)
        am = p.argmax(-1, keepdim=True)
        lg = lg.scatter_add(-1, am, bad[..., None].float() * 0.003)
    boxes = torch.rand(3, nq, 4, generator=gen)
    return lg, boxes


@pytest.mark.parametrize("nq", [1, 31, 900])
@pytest.mark.parametrize("Tn", [32, 256])
def test_ground(nq, Tn):
    from anyedit_amd import ops
    lg, boxes = _ground_inputs(nq, Tn, 1000 + nq + Tn)
    p = lg.sigmoid()
    s = p.max(-1)[0]
    assert float(torch.minimum((p - BOX_T).abs(), (p - TEXT_T).abs()).min()) >= 1e-5, "a sigmoid lies within 1e-5 of a threshold"
    pos = s[s > 0]
    assert pos.numel() == 0 or float(((pos * 100 - (pos * 100).round()).abs() / 100).min()) >= 1e-4, "a score lies within 1e-4 of a multiple of 0.01"
    dl, dbx = lg.to(DEV), boxes.to(DEV)
    W = Tn // 32

    def run():
        outs = [Guarded((3,), torch.int32), Guarded((3, nq), torch.int32), Guarded((3, nq), torch.float32), Guarded((3, nq, 4), torch.float32),
                Guarded((3, nq, W), torch.int32)]
        ops.gdino_ground(dl, dbx, BOX_T, TEXT_T, out=tuple(o.t for o in outs))
        return outs

    count, idx, scores, bx, bits = _twice(run)
    kept = []
    for b in range(3):
        ri, rs, rb, rp = R.ground(lg[b], boxes[b], BOX_T, TEXT_T)
        n = int(ri.numel())
        kept.append(n)
        assert int(count[b]) == n, f"image {b}: count {int(count[b])} against {n}"
        assert torch.equal(idx[b, :n].long(), ri), f"image {b}: kept queries or their order"
        assert torch.equal(bx[b, :n].view(torch.int32), rb.contiguous().view(torch.int32)), f"image {b}: boxes"
        assert n == 0 or float((scores[b, :n].double() - rs.double()).abs().max()) <= 2.0 ** -22, f"image {b}: scores"
        assert [str(float(v))[:4] for v in scores[b, :n]] == [str(float(v))[:4] for v in rs], f"image {b}: the 4-character scores of the phrases"
        words = (rp.view(n, W, 32).long() << torch.arange(32)).sum(-1)                # bit t % 32 of word t // 32
        got = bits[b, :n].long() & 0xFFFFFFFF
        assert torch.equal(got, words), f"image {b}: token bit sets"
        assert bool((idx[b, n:] == -1).all()) and bool((scores[b, n:] == 0).all()) and bool((bx[b, n:] == 0).all()) and bool((bits[b, n:] == 0).all()), \
            f"image {b}: the rows behind count"
    assert kept[1] == 0 and kept[2] == nq and (nq < 5 or 0 < kept[0] < nq), f"the cases must cover none / all / some kept, got {kept}"
