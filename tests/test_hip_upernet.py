"""GPU tests of the UPerNet head and the segment map: its three kernels against float64 between sentinel guards, the refusals of their entry points
and wrappers, the tiny head on the reference's stored maps and the tiny segmentor end to end from the stored images (under the project's 1.5 x
control rule on the logits, and a margin rule on the labels), the UniFormer-S widths against the restatement, batch independence, graph capture and a
weight change, the file round trip with `meta.PALETTE`, and `img2seg`.  Every kernel case launches twice into fresh guarded buffers and the two
results must be bit-identical.

Bounds (each from the arithmetic, none from what the kernels gave):
  pools       |err| <= 2^-8 |exact| + (n + 1) 2^-24 mean|x|, n the bin's area: one bf16 rounding of the mean, plus n - 1 fp32 additions (each within
              2^-24 of a partial sum no larger than sum |x|, whatever their order) and the division, 2^-24 each relative to sum |x| / n after it
  resize      tests/test_hip_dpt.py's: 2^-8 |ref| + 2^-19 T, T = the four taps' magnitudes summed plus the addend's.  There the weight carries one
              fp32 rounding and 1 - l a second; here too (the source coordinate is an integer fraction, l = rem / (2 N) is one division), the
              arithmetic is the same twelve fp32 operations.  Equal sizes without an addend: bit-equal
  argmax      labels equal the float64 argmax wherever its top-two margin exceeds 32 x 2^-24 x max |logit|: about 16 fp32 roundings per value over
              the two stages, and two values; at most 0.5 % of the pixels are excluded.  Colours equal palette[label] exactly
  models      err(HIP) <= 1.5 x err(bf16-storage control) in rel-L2 on the stride-4 logits, both against the stored or fp32 reference; every pixel
              whose HIP label differs from the reference's has a reference top-two margin below 3 e_ctl, e_ctl the control's largest absolute error
              on the resized logits (two logits can each be off by e, and HIP is allowed the project's factor 1.5 over the control); the share of
              differing pixels is at most 1.5 x the control's plus 8 pixels"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import uniformer_ref as UR  # noqa: E402
import upernet_ref as R  # noqa: E402

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


def _bits(t):
    return t.contiguous().view(torch.int16)


def _images(B, H, W, C, seed, scale=2.0):
    """bf16 [B, H, W, C], every image of the batch drawn differently (its own offset and spread)"""
    g = torch.Generator().manual_seed(seed)
    off = torch.linspace(-1.0, 1.0, B).view(B, 1, 1, 1) if B > 1 else torch.zeros(1, 1, 1, 1)
    return (torch.randn(B, H, W, C, generator=g) * scale * (1.0 + 0.5 * torch.arange(B).view(B, 1, 1, 1)) + off).to(BF)


# ------------------------------------------------------------------------------------------------------------ pools
def _pool_reference(x, scales):
    """(exact, bound) float64 [B, sum s s, C]"""
    B, H, W, C = x.shape
    x = x.to(F64)
    exact, bound = [], []
    for s in scales:
        for y0, y1 in R.pool_bins(H, s):
            for x0, x1 in R.pool_bins(W, s):
                win = x[:, y0:y1, x0:x1].reshape(B, -1, C)
                n = win.shape[1]
                m = win.mean(1)
                exact.append(m)
                bound.append(2.0 ** -8 * m.abs() + (n + 1) * 2.0 ** -24 * win.abs().mean(1))
    return torch.stack(exact, 1), torch.stack(bound, 1)


@pytest.mark.parametrize("scales", [(1, 2, 3, 6), (1,), (2, 3)])
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 2, 1, 8), (2, 4, 3, 64), (1, 7, 5, 24), (2, 6, 6, 64), (1, 16, 16, 512)])
def test_pools_vs_float64(B, H, W, C, scales):
    from anyedit_amd import ops
    x = _images(B, H, W, C, seed=H * 100 + W * 10 + C + len(scales))
    dx = x.reshape(-1, C).to(DEV)
    bins = sum(s * s for s in scales)
    got, = _twice([((B * bins, C), BF)], lambda out: ops.ppm_pool(dx, B, H, W, scales, out=out))
    exact, bound = _pool_reference(x, scales)
    ratio = float(((got.view(B, bins, C).to(F64) - exact).abs() / (bound + 1e-300)).max())
    print(f"pools B={B} {H}x{W} C={C} scales={scales}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0
    if B > 1:      # an image alone gives the rows it gives inside the batch, bit for bit
        x1 = dx[H * W:2 * H * W].clone()
        alone, = _twice([((bins, C), BF)], lambda out: ops.ppm_pool(x1, 1, H, W, scales, out=out))
        assert torch.equal(_bits(alone), _bits(got[bins:2 * bins])), "an image's rows depend on its batch"


# ------------------------------------------------------------------------------------------------------------ resize and concat
RESIZE_PAIRS = [((1, 1), (3, 2)), ((2, 1), (4, 3)), ((6, 6), (16, 16)), ((4, 3), (18, 14)), ((9, 7), (18, 14)), ((7, 9), (3, 4)), ((5, 7), (5, 7))]


def _resize_check(got, x, H, W, add, relu, what):
    xs = F.relu(x.to(F64)) if relu else x.to(F64)
    ref, mags = R.bilinear64(xs, H, W)
    if add is not None:
        ref, mags = ref + add.to(F64), mags + add.to(F64).abs()
    ratio = float(((got.to(F64) - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -19 * mags + 1e-300)).max())
    print(f"{what}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0, what
    if tuple(x.shape[1:3]) == (H, W) and add is None:
        want = xs.to(BF) if relu else x
        assert torch.equal(_bits(got), _bits(want)), f"{what}: equal sizes are a copy, bit for bit"
        assert not relu or not bool((_bits(got) < 0).any()), "no sign bit survives the ReLU"


@pytest.mark.parametrize("mode", ["plain", "relu", "add", "add_in_place", "wide_stride"])
@pytest.mark.parametrize("C", [8, 24, 512])
@pytest.mark.parametrize("src,dst", RESIZE_PAIRS)
def test_resize_vs_float64(src, dst, C, mode):
    from anyedit_amd import ops
    (h, w), (H, W), B = src, dst, 2
    x = _images(B, h, w, C, seed=h * 1000 + W * 10 + C)
    add = _images(B, H, W, C, seed=h + W + C + 5) if mode.startswith("add") else None
    dx = x.reshape(-1, C).to(DEV)
    if mode == "wide_stride":      # a source row stride wider than C, NaN in the columns beside the slice
        store = torch.full((B * h * w, C + 16), float("nan"), dtype=BF, device=DEV)
        store[:, 8:8 + C] = dx
        dx = store[:, 8:8 + C]
    da = add.reshape(-1, C).to(DEV) if add is not None else None

    def launch(out):
        if mode == "add_in_place":
            out.copy_(da)
            ops.resize_concat([(dx, h, w, 0, False)], out, B, H, W, addend=out)
        else:
            ops.resize_concat([(dx, h, w, 0, mode == "relu")], out, B, H, W, addend=da)

    got, = _twice([((B * H * W, C), BF)], launch)
    _resize_check(got.view(B, H, W, C), x, H, W, add, mode == "relu", f"resize {h}x{w}->{H}x{W} C={C} {mode}")
    one, = _twice([((H * W, C), BF)], lambda out: ops.resize_concat([(dx[h * w:].clone(), h, w, 0, mode == "relu")], out, 1, H, W,
                                                                   addend=None if da is None else da[H * W:].clone()))
    assert torch.equal(_bits(one), _bits(got[H * W:])), "an image's rows depend on its batch"


@pytest.mark.parametrize("B", [1, 2])
def test_five_sources_at_once_leave_the_other_columns_alone(B):
    """the PPM concat's shape: a copy and four resized maps, one of them read from an image-strided slice of a wider buffer as the head reads the
    pooled product; sentinel columns between and after the slices"""
    from anyedit_amd import ops
    H, W, ld = 18, 14, 96
    geo = [((18, 14), 8, 0, False), ((9, 7), 24, 16, True), ((4, 3), 8, 48, False), ((1, 1), 16, 56, True), ((2, 1), 8, 80, False)]   # size, C, col, relu
    xs = [_images(B, h, w, C, seed=10 * i + B) for i, ((h, w), C, _, _) in enumerate(geo)]
    srcs = []
    for i, (x, ((h, w), C, col, relu)) in enumerate(zip(xs, geo)):
        d = x.reshape(B, h * w, C).to(DEV)
        if i == 2:                                     # rows 5 .. 5 + h w of every image of a [B, 40, 32] buffer, columns 16 .. 24
            store = torch.full((B, 40, 32), float("nan"), dtype=BF, device=DEV)
            store[:, 5:5 + h * w, 16:16 + C] = d
            d = store[:, 5:5 + h * w, 16:16 + C]
        else:
            d = d.reshape(B * h * w, C)
        srcs.append((d, h, w, col, relu))
    got, = _twice([((B * H * W, ld), BF)], lambda out: ops.resize_concat(srcs, out, B, H, W))
    written = torch.zeros(ld, dtype=torch.bool)
    for x, ((h, w), C, col, relu) in zip(xs, geo):
        _resize_check(got[:, col:col + C].reshape(B, H, W, C), x, H, W, None, relu, f"five sources: {h}x{w} C={C} at column {col}")
        written[col:col + C] = True
    assert int((~written).sum()) == 32
    assert bool((got[:, ~written].contiguous().view(torch.uint8) == SENT).all()), "a column outside the slices was written"


# ------------------------------------------------------------------------------------------------------------ argmax
ARGMAX_CASES = [((1, 1), (4, 4), (4, 4), 2), ((18, 14), (72, 56), (72, 56), 150), ((18, 14), (72, 56), (101, 83), 150), ((10, 26), (40, 104), (23, 57), 150),
                ((3, 2), (12, 8), (12, 8), 256), ((3, 2), (12, 8), (7, 9), 2), ((5, 4), (20, 16), (20, 16), 5)]


@pytest.mark.parametrize("with_palette", [False, True])
@pytest.mark.parametrize("src,mid,out,ncls", ARGMAX_CASES)
def test_argmax_vs_float64(src, mid, out, ncls, with_palette):
    from anyedit_amd import ops
    (h, w), (Ho, Wo), B = src, out, 2
    g = torch.Generator().manual_seed(h * 100 + Wo + ncls)
    logits = torch.randn(B, h, w, ncls, generator=g) * 5.0 + torch.randn(1, 1, 1, ncls, generator=g)
    ld = (ncls + 3) // 4 * 4 + 4
    store = torch.full((B * h * w, ld), float("inf"))               # + inf beside the classes: a kernel that reads a pad column labels it
    store[:, :ncls] = logits.reshape(-1, ncls)
    dl = store.to(DEV)
    pal = torch.randint(0, 256, (ncls, 3), generator=g, dtype=torch.uint8)
    specs = [((B, Ho, Wo), torch.uint8)] + ([((B, Ho, Wo, 3), torch.uint8)] if with_palette else [])
    outs = _twice(specs, lambda lab, col=None: ops.seg_argmax(dl, ncls, B, h, w, mid, out, palette=pal.to(DEV) if with_palette else None, labels=lab, colours=col))
    full = R.bilinear64(R.bilinear64(logits.to(F64), *mid)[0], *out)[0]                       # [B, Ho, Wo, ncls]; the second stage is exact at equal sizes
    top = full.topk(2, dim=-1).values
    clear = (top[..., 0] - top[..., 1]) > 32 * 2.0 ** -24 * float(logits.abs().max())
    excluded = float((~clear).float().mean())
    labels = outs[0].long()
    wrong = int((labels != full.argmax(-1))[clear].sum())
    print(f"argmax {src}->{mid}->{out} ncls={ncls}: {100 * excluded:.3f} % excluded, {wrong} wrong labels, {len(labels.unique())} distinct")
    assert int(labels.max()) < ncls, "a pad column was read"
    assert excluded <= 0.005 and wrong == 0
    if with_palette:
        assert torch.equal(outs[1], pal[labels]), "colours are palette[label]"


def test_argmax_of_equal_logits_is_the_lower_index():
    """identity sizes (every weight is exactly 1 or 0): planted equal maxima within a lane's four classes, across lanes, and at the last class"""
    from anyedit_amd import ops
    h, w, ncls = 6, 5, 256
    logits = torch.randn(1, h, w, ncls, generator=torch.Generator().manual_seed(0))
    plants = {(0, 0): (4, 5), (1, 2): (3, 200), (2, 4): (77, 149, 255), (5, 4): (0, 255), (3, 3): (254, 255), (4, 1): (129, 130, 131)}
    for (y, x), classes in plants.items():
        logits[0, y, x, list(classes)] = 9.0
    got, = _twice([((1, h, w), torch.uint8)], lambda lab: ops.seg_argmax(logits.reshape(-1, ncls).to(DEV), ncls, 1, h, w, (h, w), (h, w), labels=lab))
    assert torch.equal(got.long(), logits.argmax(-1)), "identity sizes reproduce the plain argmax"
    for (y, x), classes in plants.items():
        assert int(got[0, y, x]) == min(classes), ((y, x), classes, int(got[0, y, x]))


# ------------------------------------------------------------------------------------------------------------ refusals
def _refused(rc, buf, word):
    from anyedit_amd import _lib
    torch.cuda.synchronize()
    msg = _lib.lib.ae_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)
    assert bool((buf == SENT).all()), "a refused call wrote to its output"


def test_entry_points_refuse_without_launching():
    from anyedit_amd import _lib
    lib = _lib.lib
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    longs = lambda *v: (ctypes.c_long * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    x = torch.zeros(2 * 4 * 4, 16, dtype=BF, device=DEV)
    buf, out = _guarded((2 * 50, 16), BF)
    sc = ints(1, 2, 3, 6)
    _refused(lib.ae_ppm_pool_rows_bf16(None, p(out), 2, 4, 4, 16, sc, 4, s), buf, "null pointer")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, 4, 16, None, 4, s), buf, "null pointer")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 0, 4, 4, 16, sc, 4, s), buf, "bad sizes")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, -1, 16, sc, 4, s), buf, "bad sizes")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, 4, 12, sc, 4, s), buf, "multiple of 8")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, 4, 16, ints(1, 2, 3, 6, 8), 5, s), buf, "5 scales")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, 4, 16, sc, 0, s), buf, "0 scales")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, 4, 16, ints(1, 9), 2, s), buf, "pool scale 9")
    _refused(lib.ae_ppm_pool_rows_bf16(p(x), p(out), 2, 4, 4, 16, ints(0), 1, s), buf, "pool scale 0")
    _refused(lib.ae_ppm_pool_rows_bf16(p(out), p(out), 2, 4, 4, 16, ints(1), 1, s), buf, "must not alias x")

    buf, dst = _guarded((2 * 8 * 8, 32), BF)

    def rc(src=x, h=4, w=4, c=16, ld=16, img=256, col=0, relu=0, n=1, add=None, ld_add=0, d=dst, ld_dst=32, B=2, H=8, W=8, arrays=None):
        a = arrays or (ptrs(*[p(src)] * n), ints(*[h] * n), ints(*[w] * n), ints(*[c] * n), longs(*[ld] * n), longs(*[img] * n),
                       ints(*[col + 16 * i for i in range(n)]), ints(*[relu] * n))
        return lib.ae_resize_concat_rows_bf16(*a, n, None if add is None else p(add), ld_add, None if d is None else p(d), ld_dst, B, H, W, s)

    _refused(rc(d=None), buf, "null pointer")
    _refused(rc(arrays=(ptrs(None), ints(4), ints(4), ints(16), longs(16), longs(256), ints(0), ints(0))), buf, "null pointer")
    _refused(rc(n=6), buf, "6 sources")
    _refused(rc(n=0, arrays=(ptrs(p(x)), ints(4), ints(4), ints(16), longs(16), longs(256), ints(0), ints(0))), buf, "0 sources")
    _refused(rc(B=0), buf, "bad sizes")
    _refused(rc(H=0), buf, "bad sizes")
    _refused(rc(h=0), buf, "bad sizes of source 0")
    _refused(rc(c=12), buf, "multiple of 8")
    _refused(rc(ld=8), buf, "row stride")
    _refused(rc(ld_dst=36), buf, "row stride")
    _refused(rc(img=100), buf, "image stride")
    _refused(rc(col=24), buf, "does not fit")
    _refused(rc(col=4), buf, "does not fit")
    _refused(rc(n=2, arrays=(ptrs(p(x), p(x)), ints(4, 4), ints(4, 4), ints(16, 16), longs(16, 16), longs(256, 256), ints(0, 8), ints(0, 0))), buf, "overlap")
    _refused(rc(n=2, add=x, ld_add=16), buf, "single source")
    _refused(rc(src=dst, h=8, w=8, ld=32, img=2048), buf, "must not alias source 0")
    _refused(rc(add=dst[1:], ld_add=32), buf, "the destination's slice itself or a buffer apart")
    _refused(rc(add=x, ld_add=8), buf, "addend must be 16-byte aligned")

    logits = torch.zeros(2 * 4 * 4, 152, device=DEV)
    pal = torch.zeros(150, 3, dtype=torch.uint8, device=DEV)
    buf, lab = _guarded((2, 16, 16), torch.uint8)
    cbuf, col = _guarded((2, 16, 16, 3), torch.uint8)
    am = lambda lg=logits, ld=152, n=150, pl=None, lb=lab, cl=None, B=2, h=4, w=4, Hm=16, Wm=16, Ho=16, Wo=16: lib.ae_seg_argmax_u8(
        None if lg is None else p(lg), ld, n, None if pl is None else p(pl), None if lb is None else p(lb), None if cl is None else p(cl), B, h, w, Hm, Wm, Ho, Wo, s)
    _refused(am(lg=None), buf, "null pointer")
    _refused(am(lb=None), buf, "null pointer")
    _refused(am(pl=pal), buf, "go together")
    _refused(am(cl=col), cbuf, "go together")
    _refused(am(n=257, ld=260), buf, "257 classes")
    _refused(am(n=0), buf, "0 classes")
    _refused(am(ld=148), buf, "row stride")
    _refused(am(ld=150, n=150), buf, "row stride")
    _refused(am(B=0), buf, "bad sizes")
    _refused(am(Hm=0), buf, "bad sizes")
    _refused(am(Wo=20000), buf, "bad sizes")
    assert bool((cbuf == SENT).all())


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from anyedit_amd import ops
    z = lambda *sh, dt=BF: torch.zeros(*sh, dtype=dt, device=DEV)
    with pytest.raises(ValueError, match="pool scales"):
        ops.ppm_pool(z(16, 8), 1, 4, 4, (1, 2, 3, 6, 8))
    with pytest.raises(ValueError, match="pool scales"):
        ops.ppm_pool(z(16, 8), 1, 4, 4, (9,))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.ppm_pool(z(16, 12), 1, 4, 4, (1,))
    with pytest.raises(ValueError, match="expected contiguous rows"):
        ops.ppm_pool(z(15, 8), 1, 4, 4, (1,))
    with pytest.raises(TypeError):
        ops.ppm_pool(z(16, 8, dt=torch.float32), 1, 4, 4, (1,))
    dst = z(64, 32)
    with pytest.raises(ValueError, match="sources per launch"):
        ops.resize_concat([(z(16, 8), 4, 4, 0, False)] * 6, dst, 1, 8, 8)
    with pytest.raises(ValueError, match="do not fit"):
        ops.resize_concat([(z(16, 16), 4, 4, 24, False)], dst, 1, 8, 8)
    with pytest.raises(ValueError, match="overlaps an earlier one"):
        ops.resize_concat([(z(16, 16), 4, 4, 0, False), (z(16, 16), 4, 4, 8, False)], dst, 1, 8, 8)
    with pytest.raises(ValueError, match="single source"):
        ops.resize_concat([(z(16, 8), 4, 4, 0, False), (z(16, 8), 4, 4, 8, False)], dst, 1, 8, 8, addend=z(64, 8))
    with pytest.raises(ValueError, match="expected rows"):
        ops.resize_concat([(z(15, 8), 4, 4, 0, False)], dst, 1, 8, 8)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.resize_concat([(z(16, 12), 4, 4, 0, False)], dst, 1, 8, 8)
    with pytest.raises(Exception, match="must not alias source 0"):
        ops.resize_concat([(dst, 8, 8, 0, False)], dst, 1, 8, 8)
    with pytest.raises(ValueError, match="classes"):
        ops.seg_argmax(z(16, 260, dt=torch.float32), 257, 1, 4, 4, (8, 8))
    with pytest.raises(ValueError, match="row stride"):
        ops.seg_argmax(z(16, 150, dt=torch.float32), 150, 1, 4, 4, (8, 8))
    with pytest.raises(ValueError, match="palette must be"):
        ops.seg_argmax(z(16, 152, dt=torch.float32), 150, 1, 4, 4, (8, 8), palette=z(149, 3, dt=torch.uint8))
    with pytest.raises(ValueError, match="without a palette"):
        ops.seg_argmax(z(16, 152, dt=torch.float32), 150, 1, 4, 4, (8, 8), colours=z(1, 8, 8, 3, dt=torch.uint8))
    with pytest.raises(TypeError):
        ops.seg_argmax(z(16, 152), 150, 1, 4, 4, (8, 8))


# ------------------------------------------------------------------------------------------------------------ models
def _model(geo, hgeo, bsd, hsd, palette=None):
    from anyedit_amd.checkpoints import load_segmentor
    from anyedit_amd.uniformer import UniFormer
    from anyedit_amd.uniformer.upernet import EncoderDecoder, UPerHead
    backbone = UniFormer(layers=list(geo["layers"]), embed_dim=list(geo["embed_dim"]), head_dim=geo["head_dim"])
    head = UPerHead(pool_scales=hgeo["pool_scales"], in_channels=list(hgeo["in_channels"]), channels=hgeo["channels"], num_classes=hgeo["num_classes"],
                    norm_cfg=dict(type="BN", requires_grad=True))
    model = EncoderDecoder(backbone, head, test_cfg=dict(mode="whole"), palette=palette)
    load_segmentor(model, dict({"backbone." + k: v for k, v in bsd.items()}, **{"decode_head." + k: v for k, v in hsd.items()}))
    return model.to(DEV)


@pytest.fixture(scope="module")
def tiny():
    bsd, hsd = sub_sd(load_golden("uniformer_tiny_w"), "w."), sub_sd(load_golden("upernet_tiny_w"), "w.")
    pal = load_golden("ade_palette")["palette"]
    return _model(UR.TINY, R.TINY_HEAD, bsd, hsd, palette=pal), bsd, hsd, load_golden("upernet_tiny_io"), load_golden("uniformer_tiny_io"), pal


def _rows_of(maps):
    return [(m.permute(0, 2, 3, 1).reshape(-1, m.shape[1]).to(BF).contiguous().to(DEV), m.shape[2], m.shape[3]) for m in maps]


def _judge(label, hip_logits, ctl_logits, ref_logits, hip_labels, mid, oris, ref_labels=None):
    """the two rules of the module docstring; hip_labels: {ori: uint8 [B, Ho, Wo] on the CPU}; ref_labels: the reference's stored labels likewise
    (without them: the restatement's simple_test of ref_logits)"""
    e_hip, e_ctl = rel_l2(hip_logits, ref_logits), rel_l2(ctl_logits, ref_logits)
    report = [f"{label} logits {tuple(ref_logits.shape)}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}"]
    ok = e_hip <= 1.5 * e_ctl
    for ori in oris:
        full = R.resize_twice(ref_logits, mid, ori)
        full_ctl = R.resize_twice(ctl_logits, mid, ori)
        e_abs = float((full_ctl - full).abs().max())
        want, margin = ref_labels[ori].long() if ref_labels else full.softmax(1).argmax(1), R.top_two_margin(full)
        diff_hip, diff_ctl = hip_labels[ori].long() != want, full_ctl.argmax(1) != want
        worst = float(margin[diff_hip].max()) if bool(diff_hip.any()) else 0.0
        n_hip, n_ctl = int(diff_hip.sum()), int(diff_ctl.sum())
        report.append(f"{label} labels at {ori}: HIP differs at {n_hip} of {want.numel()} pixels (control {n_ctl}, ratio {n_hip / max(n_ctl, 1):.2f}); largest "
                      f"margin there {worst:.3e} against 3 e_ctl = {3 * e_abs:.3e}")
        ok &= worst < 3 * e_abs and n_hip <= 1.5 * n_ctl + 8
    print("\n".join(report))
    assert ok, "\n".join(report)


def _stored_labels(io, name, oris):
    return {ori: T(io[f"labels.{name}.{ori[0]}x{ori[1]}"]) for ori in oris}


@pytest.mark.parametrize("B,H,W", UR.TINY_SIZES)
def test_tiny_head_on_the_stored_maps(tiny, B, H, W):
    from anyedit_amd import ops
    model, _, hsd, io, bio, pal = tiny
    name = f"{B}x{H}x{W}"
    maps = [T(bio[f"out.{name}.{k}"]) for k in range(4)]
    rows, h, w = model.decode_head.forward_rows(_rows_of(maps), B)
    assert (h, w) == (H // 4, W // 4) and rows.dtype == torch.float32 and rows.shape[0] == B * h * w and rows.shape[1] >= 150
    hip = rows[:, :150].reshape(B, h, w, 150).permute(0, 3, 1, 2).cpu()
    assert torch.equal(model.decode_head(_rows_of(maps), B).cpu(), hip)
    oris = [(H, W), R.SECOND_ORI[name]]
    labels = {}
    for ori in oris:
        lab, col = ops.seg_argmax(rows, 150, B, h, w, (H, W), ori, palette=torch.from_numpy(pal).to(DEV))
        labels[ori] = lab.cpu()
        assert torch.equal(col.cpu(), torch.from_numpy(pal)[labels[ori].long()])
    _judge(f"head {name}", hip, R.head_control(hsd, maps, R.TINY_HEAD["pool_scales"]), T(io["logits." + name]), labels, (H, W), oris, _stored_labels(io, name, oris))


@pytest.mark.parametrize("B,H,W", UR.TINY_SIZES)
def test_tiny_segmentor_end_to_end(tiny, B, H, W):
    model, bsd, hsd, io, bio, pal = tiny
    name = f"{B}x{H}x{W}"
    x = T(bio["x." + name])
    rows, h, w = model.encode_decode_rows(x.to(DEV))
    hip = rows[:, :150].reshape(B, h, w, 150).permute(0, 3, 1, 2).cpu()
    oris = [(H, W), R.SECOND_ORI[name]]
    labels = {ori: model.simple_test(x.to(DEV), ori).cpu() for ori in oris}
    assert torch.equal(model.simple_test(x.to(DEV)).cpu(), labels[(H, W)]), "ori_shape defaults to the input's size"
    ctl = R.head_control(hsd, UR.control(bsd, x, UR.TINY["head_dim"]), R.TINY_HEAD["pool_scales"])
    _judge(f"end to end {name}", hip, ctl, T(io["logits." + name]), labels, (H, W), oris, _stored_labels(io, name, oris))


def test_uniformer_s_widths_vs_restatement():
    """The real widths (backbone 64, 128, 320, 512, head channels 512, 150 classes) with layers (1, 1, 2, 1), one 96x64 image, seeded weights, against
    the fp32 restatement on the CPU."""
    bsd = UR.seeded_state_dict(UR.WIDE["layers"], UR.WIDE["embed_dim"], UR.WIDE["head_dim"], seed=1)
    hsd = R.seeded_head_state_dict(seed=2, **R.WIDE_HEAD)
    x = UR.smooth_pixels(1, 96, 64, seed=7)
    ref = R.head_forward(hsd, UR.forward(bsd, x, UR.WIDE["head_dim"]))
    assert tuple(ref.shape) == (1, 150, 24, 16)
    ctl = R.head_control(hsd, UR.control(bsd, x, UR.WIDE["head_dim"]))
    model = _model(UR.WIDE, R.WIDE_HEAD, bsd, hsd)
    rows, h, w = model.encode_decode_rows(x.to(DEV))
    assert rows.shape[1] == 152
    hip = rows[:, :150].reshape(1, h, w, 150).permute(0, 3, 1, 2).cpu()
    _judge("S widths 96x64", hip, ctl, ref, {(96, 64): model.simple_test(x.to(DEV)).cpu()}, (96, 64), [(96, 64)])


def test_an_image_does_not_depend_on_its_batch(tiny):
    model, _, _, _, bio, _ = tiny
    x = T(bio["x.2x64x48"]).to(DEV)
    both, h, w = model.encode_decode_rows(x)
    one, _, _ = model.encode_decode_rows(x[1:2].clone())
    assert torch.equal(both[h * w:], one), "running an image with a neighbour changed its logits"
    assert not torch.equal(both[:h * w], both[h * w:])
    assert torch.equal(model.simple_test(x, (45, 67))[1:2], model.simple_test(x[1:2].clone(), (45, 67)))


def test_forward_is_capturable_and_follows_a_weight_change(tiny):
    model, _, _, _, bio, _ = tiny
    static = T(bio["x.1x72x56"]).to(DEV)
    run = lambda: (model.encode_decode_rows(static)[0], *model.simple_test(static, (101, 83), want_colours=True))
    first = [t.clone() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream: the segmentor only ever uses the current one
        out = run()
    new = UR.smooth_pixels(1, 72, 56, seed=11).to(DEV)
    static.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    before, mem = torch.cuda.memory_stats(DEV)["allocation.all.allocated"], torch.cuda.memory_allocated(DEV)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before and torch.cuda.memory_allocated(DEV) == mem, "a replay allocated"
    eager = [t.clone() for t in run()]
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager)), "graph replay differs from the eager forward of the same image"
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert not torch.equal(replayed[0], first[0])
    # in-place changes of a BatchNorm statistic, a convolution and the classifier: the next eager call refolds / repacks and follows them
    head = model.decode_head
    for p in (head.fpn_convs[0].bn.running_var, head.psp_modules[2][1].bn.running_mean, head.bottleneck.conv.weight, head.lateral_convs[1].bn.weight,
              head.conv_seg.bias):
        keep = p.detach().clone()
        with torch.no_grad():
            p.mul_(1.5)
        assert not torch.equal(run()[0], eager[0]), "an in-place weight change was not picked up"
        with torch.no_grad():
            p.copy_(keep)
        assert all(torch.equal(a, b) for a, b in zip(run(), eager))


def _uint8_image(H, W, seed):
    x = UR.smooth_pixels(1, H, W, seed=seed)[0]
    return ((x - x.min()) / (x.max() - x.min()) * 255).round().permute(1, 2, 0).to(torch.uint8).numpy()         # [H, W, 3]


def test_round_trip_through_a_file_with_meta_palette(tiny, tmp_path):
    model, bsd, hsd, _, bio, pal = tiny
    from anyedit_amd.uniformer import UniFormer
    from anyedit_amd.uniformer.upernet import EncoderDecoder, UPerHead
    path = str(tmp_path / "upernet_global_small.pth")
    sd = dict({"backbone." + k: v for k, v in bsd.items()}, **{"decode_head." + k: v for k, v in hsd.items()})
    sd["auxiliary_head.conv_seg.weight"] = torch.zeros(150, 8, 1, 1)
    shuffled = pal[::-1].copy()
    torch.save({"state_dict": sd, "meta": {"CLASSES": [f"c{i}" for i in range(150)], "PALETTE": shuffled.tolist()}}, path)
    geo, hg = UR.TINY, R.TINY_HEAD
    other = EncoderDecoder(dict(type="UniFormer", layers=list(geo["layers"]), embed_dim=list(geo["embed_dim"]), head_dim=geo["head_dim"]),
                           dict(type="UPerHead", pool_scales=hg["pool_scales"], in_channels=list(hg["in_channels"]), channels=hg["channels"],
                                num_classes=150, norm_cfg=dict(type="BN")), test_cfg=dict(mode="whole"), pretrained=path).to(DEV)
    assert isinstance(other.backbone, UniFormer) and isinstance(other.decode_head, UPerHead) and other.CLASSES[3] == "c3"
    x = T(bio["x.1x40x104"]).to(DEV)
    lab, col = other.simple_test(x, (23, 57), want_colours=True)
    lab0, col0 = model.simple_test(x, (23, 57), want_colours=True)
    assert torch.equal(lab, lab0)
    assert torch.equal(col.cpu(), torch.from_numpy(shuffled)[lab.cpu().long()]) and torch.equal(col0.cpu(), torch.from_numpy(pal)[lab.cpu().long()])


def test_img2seg_writes_the_palette_with_red_and_blue_exchanged(tiny, tmp_path):
    from PIL import Image
    from anyedit_amd.tools.tool import img2seg
    model, _, _, _, _, pal = tiny
    rgb = _uint8_image(64, 48, seed=5)
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "seg.png")
    Image.fromarray(rgb).save(src)
    assert img2seg(src, dst, model) == dst
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    x, ori = model.preprocess(bgr)
    assert ori == (64, 48) and tuple(x.shape) == (1, 3, 683, 512), "the keep-ratio rescale to a short side of 512"
    labels = model.simple_test(x, ori).cpu().long()[0]
    assert len(labels.unique()) >= 2
    written = np.array(Image.open(dst).convert("RGB"))
    assert written.shape == (64, 48, 3)
    assert np.array_equal(written, pal[labels.numpy()][:, :, ::-1]), "the file shows palette[label] with red and blue exchanged"
    assert np.array_equal(model.colour_image(bgr), pal[labels.numpy()])
