"""GPU tests of the HED edge detector: its kernels against float64 between sentinel guards, the tiny tower against the reference's golden at the
three stored image sizes and the full-width tower against the restatement (under the project's 1.5 x control rule), batch independence, graph
capture, and the file round trip of `img2scribble`.  Every case runs once; every kernel case launches twice into fresh guarded buffers and the
two results must be bit-identical.

Bounds (each from the arithmetic, none from what the kernels gave):
  stem   2^-8 |ref| + 2^-19 sum|terms|: one bf16 rounding of the result, plus 28 fp32 operations (the subtraction and 27 multiply-adds) at 2^-24
         each, rounded up to 32 = 2^5, relative to the sum of the absolute terms
  tail   pooled map bit-equal (a maximum of bf16 values is one of them); projection within (C + 2) 2^-24 (sum_c |r_c w_c| + |b|): C multiply-adds,
         the bias, and slack for the order of the partial sums
  fuse   logit within 2^-20 sum|terms| (16 fp32 roundings: the weights, the products, the sums, the division); the uint8 equal to the
         reference's wherever its float64 value v before truncation has |v - round(v)| > 1e-3, within 1 elsewhere, that share at most 1 %
  tower  err(HIP) <= 1.5 x err(bf16-storage control) in rel-L2, both against the stored or fp32 reference"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import hed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0xA5            # every byte of a guarded buffer before the launch
GUARD = 4096           # bytes on either side


def _guarded(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _twice(specs, launch):
    """Runs `launch(*outs)` twice on fresh guarded buffers of `specs` = [(shape, dtype), ...]: guards intact, the two results bit-identical;
    returns the results on the CPU."""
    runs = []
    for _ in range(2):
        pairs = [_guarded(s, d) for s, d in specs]
        launch(*[o for _, o in pairs])
        torch.cuda.synchronize()
        assert all(_guards_intact(b) for b, _ in pairs), "wrote outside its output"
        runs.append([o.clone().cpu() for _, o in pairs])
    for a, b in zip(*runs):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), "two launches differ"
    return runs[0]


# ------------------------------------------------------------------------------------------------------------ stem
def _stem_weights(C1, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C1, 3, 3, 3, generator=g) * 0.2, torch.randn(C1, generator=g) * 8.0, torch.tensor(R.NORM)


def _stem_inputs(form, B, H, W, seed):
    """(device tensor as the kernel takes it, the same values as float64 [B, 3, H, W])"""
    g = torch.Generator().manual_seed(seed)
    if form == "u8":
        x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        return x.to(DEV), x.permute(0, 3, 1, 2).to(F64)
    x = torch.rand(B, 3, H, W, generator=g) * 255.0
    if B == 2:                                  # the same values behind other strides: channels-last memory
        return x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), x.to(F64)
    return x.to(DEV), x.to(F64)


@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("C1", [8, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (17, 33), (50, 38)])
@pytest.mark.parametrize("B", [1, 2])
def test_stem_vs_float64(B, H, W, C1, form):
    from anyedit_amd import ops
    w, bias, norm = _stem_weights(C1, seed=C1 + H)
    dx, x64 = _stem_inputs(form, B, H, W, seed=B * 1000 + H * 10 + W)
    dw, db, dn = w.to(DEV), bias.to(DEV), norm.to(DEV)
    got, = _twice([((B * H * W, C1), BF)], lambda out: ops.hed_stem(dx, dn, dw, db, out=out))
    h = x64 - norm.to(F64).view(1, 3, 1, 1)
    ref = F.relu(F.conv2d(h, w.to(F64), bias.to(F64), padding=1))
    terms = F.conv2d(h.abs(), w.to(F64).abs(), bias.to(F64).abs(), padding=1)
    ref, terms = (t.permute(0, 2, 3, 1).reshape(B * H * W, C1) for t in (ref, terms))
    ratio = float(((got.to(F64) - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -19 * terms)).max())
    print(f"stem {form} B={B} {H}x{W} C1={C1}: worst |err| / bound = {ratio:.3f}; zeros {100 * float((got == 0).float().mean()):.0f} %")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0
    assert ref.numel() < 64 or (bool((ref > 0).any()) and bool((ref == 0).any())), "both sides of the ReLU"


@pytest.mark.parametrize("form", ["u8", "f32"])
def test_stem_pads_the_normalised_image_with_zeros(form):
    """An image equal to the integer-valued norm everywhere: x - norm is 0 at every pixel and 0 outside, so every output is exactly
    bf16(relu(bias)), the border rows and columns included.  A kernel that pads x with zeros (-norm * w outside) fails on the border."""
    from anyedit_amd import ops
    B, H, W, C1 = 2, 9, 7, 16
    w, bias, norm = _stem_weights(C1, seed=1)
    img = norm.view(1, 1, 1, 3).expand(B, H, W, 3)
    dx = img.to(torch.uint8).contiguous().to(DEV) if form == "u8" else img.permute(0, 3, 1, 2).contiguous().to(DEV)
    got, = _twice([((B * H * W, C1), BF)], lambda out: ops.hed_stem(dx, norm.to(DEV), w.to(DEV), bias.to(DEV), out=out))
    want = F.relu(bias).to(BF).view(1, C1).expand(B * H * W, C1)
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))


def test_relu_in_place():
    from anyedit_amd import ops
    for n in (1, 7, 8, 1000, 64 * 1024 + 13):
        x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3).to(BF)
        got, = _twice([((n,), BF)], lambda out: (out.copy_(x.to(DEV)), ops.relu_(out)))
        assert torch.equal(got.view(torch.int16), F.relu(x.float()).to(BF).view(torch.int16)), n


# ------------------------------------------------------------------------------------------------------------ block tail
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("C", [8, 64, 200, 512])
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (7, 6), (33, 47)])
@pytest.mark.parametrize("B", [1, 2])
def test_tail_vs_float64(B, H, W, C, pool):
    from anyedit_amd import ops
    g = torch.Generator().manual_seed(C * 100 + H * 10 + B)
    y = (torch.randn(B * H * W, C, generator=g) * 3.0).to(BF)
    wp, bp = torch.randn(C, generator=g) / C ** 0.5, torch.randn(1, generator=g)
    assert bool((y.float() < 0).any()) and bool((y.float() > 0).any())
    dy, dw, db = y.to(DEV), wp.to(DEV), bp.to(DEV)
    specs = [((B, H, W), torch.float32)] + ([((B * (H // 2) * (W // 2), C), BF)] if pool else [])
    outs = _twice(specs, lambda proj, pooled=None: ops.hed_tail(dy, dw, db, B, H, W, pool=pool, proj=proj, pooled=pooled))
    r = F.relu(y.float()).view(B, H, W, C)
    terms = r.to(F64) * wp.to(F64)
    ref = terms.sum(-1) + bp.to(F64)
    bound = (C + 2) * 2.0 ** -24 * (terms.abs().sum(-1) + bp.to(F64).abs())
    ratio = float(((outs[0].to(F64) - ref).abs() / bound).max())
    print(f"tail B={B} {H}x{W} C={C} pool={pool}: projection worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(outs[0]).all() and ratio <= 1.0
    if pool:
        want = F.max_pool2d(r.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).reshape(-1, C).to(BF)
        assert torch.equal(outs[1].view(torch.int16), want.contiguous().view(torch.int16)), "pooled map differs from max_pool2d(relu(y))"


# ------------------------------------------------------------------------------------------------------------ fuse
@pytest.mark.parametrize("invert", [True, False])
@pytest.mark.parametrize("H,W", [(16, 16), (17, 31), (50, 38), (33, 47)])
@pytest.mark.parametrize("B", [1, 2])
def test_fuse_vs_float64(B, H, W, invert):
    from anyedit_amd import ops
    sides = R.smooth_sides(B, H, W, seed=H * 100 + W + B)
    ds = [s.to(DEV) for s in sides]
    got, logit = _twice([((B, H, W), torch.uint8), ((B, H, W), torch.float32)], lambda out, lg: ops.hed_fuse(ds, invert=invert, out=out, logits=lg))
    only, = _twice([((B, H, W), torch.uint8)], lambda out: ops.hed_fuse([s[:, 0] for s in ds], invert=invert, out=out))
    assert torch.equal(only, got), "the map must not depend on whether the logits are asked for"
    s64 = [s.to(F64) for s in sides]
    m64 = R.mean_logits(s64, H, W)
    terms = R.mean_logits([s.abs() for s in s64], H, W)
    r_logit = float(((logit.to(F64) - m64).abs() / (2.0 ** -20 * terms)).max())
    v = R.edge_value(m64)
    ref = v.to(torch.uint8)
    ref = 255 - ref if invert else ref
    plain = 255 - ref if invert else ref
    assert float(((plain >= 5) & (plain <= 250)).double().mean()) > 0.5, "the inputs saturate the map"
    near = (v - v.round()).abs() <= 1e-3
    d = (got.int() - ref.int()).abs()
    print(f"fuse B={B} {H}x{W} invert={invert}: logit worst |err| / bound = {r_logit:.3f}; pixels within 1e-3 of an integer {100 * float(near.double().mean()):.2f} %; "
          f"differing there {int((d[near] > 0).sum())}, elsewhere {int((d[~near] > 0).sum())}")
    assert r_logit <= 1.0
    assert float(near.double().mean()) <= 0.01
    assert int(d[~near].max()) == 0 and (int(d[near].max()) <= 1 if bool(near.any()) else True)


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from anyedit_amd import ops, _lib
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(_lib.AnyEditHipError, match="multiple of 8"):
        ops.hed_stem(z(1, 4, 4, 3, dt=torch.uint8), z(3), z(12, 3, 3, 3), z(12))
    with pytest.raises(TypeError):
        ops.hed_stem(z(1, 3, 4, 4, dt=BF), z(3), z(8, 3, 3, 3), z(8))
    with pytest.raises(ValueError, match="uint8"):
        ops.hed_stem(z(1, 4, 4, 4, dt=torch.uint8), z(3), z(8, 3, 3, 3), z(8))
    with pytest.raises(_lib.AnyEditHipError, match="multiple of 8"):
        ops.hed_tail(z(4, 12, dt=BF), z(12), z(1), 1, 2, 2)
    with pytest.raises(ValueError, match="no 2x2 window"):
        ops.hed_tail(z(3, 8, dt=BF), z(8), z(1), 1, 1, 3)
    with pytest.raises(ValueError, match="side map 2"):
        ops.hed_fuse([z(1, 16, 16), z(1, 8, 8), z(1, 5, 4), z(1, 2, 2), z(1, 1, 1)])
    with pytest.raises(ValueError, match="16 .. 16384"):
        ops.hed_fuse([z(1, 15 >> k, 32 >> k) for k in range(4)] + [z(1, 1, 2)])
    with pytest.raises(ValueError, match="contiguous"):
        ops.relu_(z(4, 16, dt=BF)[:, :8])


# ------------------------------------------------------------------------------------------------------------ towers
@pytest.fixture(scope="module")
def tiny():
    from anyedit_amd.hed import HEDdetector
    sd = sub_sd(load_golden("hed_tiny_w"), "w.")
    return HEDdetector(sd, device=DEV, **R.TINY), sd, load_golden("hed_tiny_io")


def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


def _tower_case(det, sd, img, ref_sides, label):
    """The five projections (fp32 __call__ form) and the mean logit map (uint8 detect form) of the HIP tower and of the control, both against
    `ref_sides`, under the control rule; the uint8 maps' differences are printed."""
    H, W = img.shape[:2]
    x = R.to_nchw(img)
    ctl = R.control(sd, x)
    hip = det.netNetwork(x.to(DEV))
    report, ok = [], True
    for k in range(5):
        assert tuple(hip[k].shape) == tuple(ref_sides[k].shape) and hip[k].dtype == torch.float32
        ok &= _judge(f"{label} projection {k + 1}", hip[k], ctl[k], ref_sides[k], report)
    edge, logit = det.detect(torch.from_numpy(img).to(DEV).unsqueeze(0), want_logits=True)
    m_ref = R.mean_logits(ref_sides, H, W)
    ok &= _judge(f"{label} mean logit map", logit, R.mean_logits(ctl, H, W), m_ref, report)
    e_ref = R.edge_map(ref_sides, H, W).int()
    for name, e in (("HIP", edge.cpu().int()), ("control", R.edge_map(ctl, H, W).int())):
        d = (e - e_ref).abs()
        report.append(f"{label} uint8 map, {name}: largest difference {int(d.max())}, differing {100 * float((d > 0).float().mean()):.1f} %")
    print("\n".join(report))
    assert ok, "\n".join(report)
    assert edge.dtype == torch.uint8 and tuple(edge.shape) == (1, H, W)


@pytest.mark.parametrize("H,W", R.TINY_SIZES)
def test_tiny_tower_vs_golden(tiny, H, W):
    det, sd, io = tiny
    _tower_case(det, sd, io[f"image.{H}x{W}"], [T(io[f"proj.{H}x{W}.{k}"]) for k in range(5)], f"{H}x{W}")


def test_full_width_tower_vs_restatement():
    """The reference geometry (64 .. 512 channels, 13 convolutions) on one 96x80 image, seeded weights with the heads rescaled on this image, against
    the fp32 restatement on the CPU."""
    from anyedit_amd.hed import HEDdetector
    H, W = 96, 80
    img = R.smooth_image(H, W, seed=7)
    sd = R.seeded_state_dict(seed=1)
    R.rescale_heads(sd, R.forward(sd, R.to_nchw(img)), H, W)
    ref = R.forward(sd, R.to_nchw(img))
    assert abs(float(R.mean_logits(ref, H, W).std()) - R.LOGIT_STD) < 1e-2
    _tower_case(HEDdetector(sd, device=DEV), sd, img, ref, "full width 96x80")


def test_a_sample_does_not_depend_on_its_batch(tiny):
    det, _, io = tiny
    a, b = io["image.64x48"], R.smooth_image(64, 48, seed=9)
    both = torch.from_numpy(np.stack([a, b])).to(DEV)
    e2, l2 = det.detect(both, want_logits=True)
    e1, l1 = det.detect(both[1:2].clone(), want_logits=True)
    assert torch.equal(e2[1:2], e1) and torch.equal(l2[1:2], l1), "running an image with a neighbour changed its map"
    assert not torch.equal(e2[0], e2[1])


def test_detect_is_capturable_and_follows_a_weight_change(tiny):
    det, sd, io = tiny
    img = torch.from_numpy(io["image.64x48"]).unsqueeze(0)
    static = img.to(DEV)
    first = det.detect(static).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        det.detect(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream: the detector only ever uses the current one
        out = det.detect(static)
    new = torch.from_numpy(R.smooth_image(64, 48, seed=11)).unsqueeze(0)
    static.copy_(new.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    before, mem = torch.cuda.memory_stats(DEV)["allocation.all.allocated"], torch.cuda.memory_allocated(DEV)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before and torch.cuda.memory_allocated(DEV) == mem, "a replay allocated"
    assert torch.equal(out, replayed)
    eager = det.detect(new.to(DEV))
    assert torch.equal(replayed, eager), "graph replay differs from the eager detect of the same image"
    assert not torch.equal(replayed, first)
    # an in-place weight change: the next eager call repacks and follows it; the restored weights give the first map back
    p = det.netNetwork.block2.convs[1].weight
    keep = p.detach().clone()
    with torch.no_grad():
        p.mul_(-0.5)
    changed = det.detect(new.to(DEV)).clone()
    assert not torch.equal(changed, eager), "an in-place weight change was not picked up"
    with torch.no_grad():
        p.copy_(keep)
    assert torch.equal(det.detect(new.to(DEV)), eager)


def test_img2scribble_round_trip(tiny, tmp_path):
    """Through files: the array written equals detect_array of the image with its channel axis reversed (cv2.imread's order)."""
    from PIL import Image
    from anyedit_amd.tools.tool import img2scribble
    det, _, io = tiny
    rgb = io["image.50x38"]
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "scribble.png")
    Image.fromarray(rgb).save(src)
    assert img2scribble(src, dst, det) == dst
    back = np.array(Image.open(dst))
    want = det.detect_array(rgb[:, :, ::-1])
    assert back.dtype == np.uint8 and back.shape == (50, 38) and np.array_equal(back, want)
    assert not np.array_equal(want, det.detect_array(rgb)), "the flip must matter for this image"
