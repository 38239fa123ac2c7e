"""GPU tests of the UniFormer backbone: its three kernels against float64 between sentinel guards, the refusals of their entry points, the tiny
backbone against the reference's golden maps at the three stored image sizes and the UniFormer-S-wide one against the restatement (under the project's
1.5 x control rule), batch independence, graph capture, and the file round trip of `load_uniformer`.  Every kernel case launches twice into fresh guarded
buffers and the two results must be bit-identical.

Bounds (each from the arithmetic, none from what the kernels gave):
  dwconv      |err| <= 2^-8 |exact| + (k^2 + 2) 2^-24 (|res| + |bias| + sum |w x|): one bf16 rounding of the result, plus k^2 fp32 multiply-adds, the
              bias and the residual at 2^-24 each relative to the sum of the absolute terms.  Inputs taken as their bf16 values, weights as fp32.
  patch2      exact (a copy)
  layernorm   tests/norm_ref.py's LayerNorm bound (two-pass statistics: e_r = a, e_mu = a (1 + rho), a = 2^-16, carried through xhat gamma + beta, plus
              a times the absolute terms) with the fp32 output's 2^-24 |ref| in place of the bf16 rounding's 2^-8 |ref|; the optional bf16 rows
              within one bf16 ulp of the rounded fp32 output
  backbone    err(HIP) <= 1.5 x err(bf16-storage control) in rel-L2, both against the stored or fp32 reference, every level"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import norm_ref  # noqa: E402
import uniformer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0xA5            # every byte of a guarded buffer before the launch
GUARD = 4096           # bytes on either side (at least one filled row of every shape here)


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


# ------------------------------------------------------------------------------------------------------------ depthwise convolution
DW_SHAPES = [(1, 1, 1, 8, 3), (1, 1, 1, 8, 5), (2, 2, 3, 8, 5), (2, 5, 7, 24, 3), (3, 17, 33, 64, 5), (2, 4, 3, 320, 5), (1, 33, 17, 512, 3),
             (1, 9, 130, 320, 5),
             (1, 3, 5, 640, 5)]      # the last one: rows too wide for the k = 5 weights' LDS image, the kernel form that reads them from global memory


def _dw_operands(B, H, W, C, k, seed):
    """rows bf16 [B*H*W, C] with every image of the batch drawn differently (its own offset and spread), a second such tensor for the separate
    residual, fp32 weights [C, 1, k, k] and bias"""
    g = torch.Generator().manual_seed(seed)
    off = torch.linspace(-2.0, 2.0, B).view(B, 1, 1, 1) if B > 1 else torch.zeros(1, 1, 1, 1)
    x = (torch.randn(B, H, W, C, generator=g) * (1.0 + 0.5 * torch.arange(B).view(B, 1, 1, 1)) + off).to(BF)
    res = (torch.randn(B, H, W, C, generator=g) * 2.0 - off).to(BF)
    return x, res, torch.randn(C, 1, k, k, generator=g) / k, torch.randn(C, generator=g)


def _dw_reference(x, res, w, bias, k):
    """(exact, bound) as rows [B*H*W, C] in float64"""
    B, H, W, C = x.shape
    nchw = lambda t: t.to(F64).permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, C)
    conv = F.conv2d(nchw(x), w.to(F64), None, padding=k // 2, groups=C)
    terms = F.conv2d(nchw(x).abs(), w.to(F64).abs(), None, padding=k // 2, groups=C)
    b = bias.to(F64).view(1, C, 1, 1)
    r = nchw(res) if res is not None else torch.zeros_like(conv)
    exact = r + b + conv
    bound = 2.0 ** -8 * exact.abs() + (k * k + 2) * 2.0 ** -24 * (r.abs() + b.abs() + terms)
    return rows(exact), rows(bound)


@pytest.mark.parametrize("mode", ["plain", "res_is_x", "res_separate"])
@pytest.mark.parametrize("B,H,W,C,k", DW_SHAPES)
def test_dwconv_vs_float64(B, H, W, C, k, mode):
    from anyedit_amd import ops
    x, res, w, bias = _dw_operands(B, H, W, C, k, seed=B * 1000 + H * 10 + W + C)
    dx = x.reshape(-1, C).to(DEV)
    dres = {"plain": None, "res_is_x": dx, "res_separate": res.reshape(-1, C).to(DEV)}[mode]
    dw, db = ops.pack_dwconv(w).to(DEV), bias.to(DEV)
    got, = _twice([((B * H * W, C), BF)], lambda out: ops.dwconv(dx, dw, db, B, H, W, residual=dres, out=out))
    exact, bound = _dw_reference(x, {"plain": None, "res_is_x": x, "res_separate": res}[mode], w, bias, k)
    ratio = float(((got.to(F64) - exact).abs() / (bound + 1e-300)).max())
    print(f"dwconv B={B} {H}x{W} C={C} k={k} {mode}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0
    if B > 1:      # an image alone gives the rows it gives inside the batch, bit for bit
        sl = slice(H * W, 2 * H * W)
        x1 = dx[sl].clone()
        r1 = {"plain": None, "res_is_x": x1, "res_separate": None if dres is None else dres[sl].clone()}[mode]
        alone, = _twice([((H * W, C), BF)], lambda out: ops.dwconv(x1, dw, db, 1, H, W, residual=r1, out=out))
        assert torch.equal(_bits(alone), _bits(got[sl])), "an image's rows depend on its batch"


def test_dwconv_reads_neither_the_next_row_nor_the_next_image():
    """A single bright pixel at the last column of a row / the last row of an image: with a weight of ones and zero bias the output is the box
    filter of that pixel clipped to its own image; a kernel that pads by the row index leaks it into the next row's first columns or the next image."""
    from anyedit_amd import ops
    B, H, W, C = 2, 4, 5, 8
    for k in (3, 5):
        x = torch.zeros(B, H, W, C)
        x[0, H - 1, W - 1] = 1.0
        x[1, H - 1, 0] = 2.0
        w = torch.ones(C, 1, k, k)
        got, = _twice([((B * H * W, C), BF)], lambda out: ops.dwconv(x.reshape(-1, C).to(BF).to(DEV), ops.pack_dwconv(w).to(DEV), torch.zeros(C, device=DEV), B, H, W, out=out))
        want = F.conv2d(x.permute(0, 3, 1, 2), w, padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
        assert torch.equal(got.float(), want), k
        g4 = got.float().view(B, H, W, C)
        assert float(g4[1, 0].abs().max()) == 0.0, "image 0's last row leaked into image 1's first"
        assert float(g4[0, :, 0].abs().max()) == 0.0 and float(g4[1, :, W - 1].abs().max()) == 0.0, "a map row's end leaked into the next row's start"


# ------------------------------------------------------------------------------------------------------------ patch gather
@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (2, 5, 7, 16), (2, 3, 3, 128), (1, 9, 4, 320)])
def test_patch2_rows_exact(B, H, W, C):
    from anyedit_amd import ops
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * 10 + W)).to(BF)
    h, w = H // 2, W // 2
    got, = _twice([((B * h * w, 4 * C), BF)], lambda out: ops.patch2_rows(x.reshape(-1, C).to(DEV), B, H, W, out=out))
    want = x[:, :2 * h, :2 * w].reshape(B, h, 2, w, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 4 * C)
    assert torch.equal(_bits(got), _bits(want))
    # the column order is pack_patch2's: the product equals the strided convolution
    wt = torch.randn(8, C, 2, 2, generator=torch.Generator().manual_seed(1)).to(BF).float()
    prod = got.to(F64) @ ops.pack_patch2(wt).to(F64).t()
    conv = F.conv2d(x.to(F64).permute(0, 3, 1, 2), wt.to(F64), stride=2).permute(0, 2, 3, 1).reshape(-1, 8)
    assert float((prod - conv).abs().max()) <= 1e-12 * max(float(conv.abs().max()), 1.0)


# ------------------------------------------------------------------------------------------------------------ output LayerNorm
@pytest.mark.parametrize("want_rows", [False, True])
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 3, 5, 64), (1, 7, 9, 320), (2, 4, 4, 512), (1, 1, 130, 128)])
def test_layernorm_rows_nchw_vs_float64(B, H, W, C, want_rows):
    """norm_ref.forward gives y and bnd = 2^-8 |y| + rest for a bf16 result (LayerNorm = GroupNorm with B = rows, HW = 1, one group; two-pass
    statistics).  The fp32 map keeps `rest` (the statistics' allowances carried through xhat gamma + beta, and a times the absolute terms) and pays
    2^-24 |y| for its own rounding: bound = bnd - 2^-8 |y| + 2^-24 |y|.  One row is constant (variance 0)."""
    from anyedit_amd import ops
    eps = 1e-6
    gen = torch.Generator().manual_seed(C + H * W)
    M = B * H * W
    x = norm_ref.make_x(gen, M, 1, C, 1, const_group=True)
    gamma, beta = norm_ref.make_affine(gen, C)
    assert bool((x.float().std(-1) == 0).any()), "a constant row"
    dx, dg, db = x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV)
    specs = [((B, C, H, W), torch.float32)] + ([((M, C), BF)] if want_rows else [])
    outs = _twice(specs, lambda out, rows=None: ops.layernorm_rows_nchw(dx, dg, db, eps, B, H, W, out=out, rows=rows))
    f = norm_ref.forward(x, gamma, beta, 1, eps, 0, False)
    y, bnd = f["y"].reshape(M, C), f["bnd"].reshape(M, C)
    bnd = bnd - 2.0 ** -8 * y.abs() + 2.0 ** -24 * y.abs()
    got = outs[0].permute(0, 2, 3, 1).reshape(M, C)
    ratio = norm_ref.check_elements(got, y, bnd, f"layernorm_rows_nchw B={B} {H}x{W} C={C}")
    print(f"layernorm_rows_nchw B={B} {H}x{W} C={C} rows={want_rows}: worst |err| / bound = {ratio:.3f}")
    if want_rows:
        d = (_bits(outs[1]).int() - _bits(got.to(BF)).int()).abs()
        print(f"   bf16 rows: {int((d > 0).sum())} of {d.numel()} differ from the rounded fp32 output, at most {int(d.max())} ulp")
        assert int(d.max()) <= 1


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
    z = lambda *sh, dt=BF: torch.zeros(*sh, dtype=dt, device=DEV)
    x, w3, w4, b = z(2 * 4 * 4, 16), z(9, 16, dt=torch.float32), z(16, 16, dt=torch.float32), z(16, dt=torch.float32)
    buf, out = _guarded((2 * 4 * 4, 16), BF)
    p = lambda t: t.data_ptr()
    _refused(lib.ae_dwconv_rows_bf16(None, p(w3), p(b), None, p(out), 2, 4, 4, 16, 3, s), buf, "null pointer")
    _refused(lib.ae_dwconv_rows_bf16(p(x), p(w3), p(b), None, None, 2, 4, 4, 16, 3, s), buf, "null pointer")
    _refused(lib.ae_dwconv_rows_bf16(p(x), p(w3), p(b), None, p(out), 0, 4, 4, 16, 3, s), buf, "bad sizes")
    _refused(lib.ae_dwconv_rows_bf16(p(x), p(w3), p(b), None, p(out), 2, -4, 4, 16, 3, s), buf, "bad sizes")
    _refused(lib.ae_dwconv_rows_bf16(p(x), p(w3), p(b), None, p(out), 2, 4, 4, 12, 3, s), buf, "multiple of 8")
    _refused(lib.ae_dwconv_rows_bf16(p(x), p(w4), p(b), None, p(out), 2, 4, 4, 16, 4, s), buf, "k=4 is not built")
    _refused(lib.ae_dwconv_rows_bf16(p(x), p(w4), p(b), None, p(out), 2, 4, 4, 16, 7, s), buf, "k=7 is not built")
    _refused(lib.ae_dwconv_rows_bf16(p(out), p(w3), p(b), None, p(out), 2, 4, 4, 16, 3, s), buf, "must not alias x")
    _refused(lib.ae_patch2_rows_bf16(None, p(out), 2, 4, 4, 16, s), buf, "null pointer")
    _refused(lib.ae_patch2_rows_bf16(p(x), p(out), 2, 1, 4, 16, s), buf, "below the 2x2 patch")
    _refused(lib.ae_patch2_rows_bf16(p(x), p(out), 2, 4, 1, 16, s), buf, "below the 2x2 patch")
    _refused(lib.ae_patch2_rows_bf16(p(x), p(out), 0, 4, 4, 16, s), buf, "bad sizes")
    _refused(lib.ae_patch2_rows_bf16(p(x), p(out), 2, 4, 4, 20, s), buf, "multiple of 8")
    fbuf, fout = _guarded((2, 16, 4, 4), torch.float32)
    _refused(lib.ae_layernorm_rows_nchw(p(x), None, p(b), 1e-6, p(fout), None, 2, 4, 4, 16, s), fbuf, "null pointer")
    _refused(lib.ae_layernorm_rows_nchw(p(x), p(b), p(b), 1e-6, None, p(out), 2, 4, 4, 16, s), buf, "null pointer")
    _refused(lib.ae_layernorm_rows_nchw(p(x), p(b), p(b), 1e-6, p(fout), None, 2, 0, 4, 16, s), fbuf, "bad sizes")
    _refused(lib.ae_layernorm_rows_nchw(p(x), p(b), p(b), 1e-6, p(fout), None, 2, 4, 4, 12, s), fbuf, "multiple of 8")
    _refused(lib.ae_layernorm_rows_nchw(p(x), p(b), p(b), 1e-6, p(fout), None, 1, 1, 1, 2048, s), fbuf, "at most 1024")


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from anyedit_amd import ops
    z = lambda *sh, dt=BF: torch.zeros(*sh, dtype=dt, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.dwconv(z(4, 12), z(9, 12, dt=torch.float32), z(12, dt=torch.float32), 1, 2, 2)
    with pytest.raises(ValueError, match="k in"):
        ops.dwconv(z(4, 8), z(16, 8, dt=torch.float32), z(8, dt=torch.float32), 1, 2, 2)
    x = z(4, 8)
    with pytest.raises(Exception, match="must not alias x"):
        ops.dwconv(x, z(9, 8, dt=torch.float32), z(8, dt=torch.float32), 1, 2, 2, out=x)
    with pytest.raises(ValueError, match="below the 2x2 patch"):
        ops.patch2_rows(z(3, 8), 1, 1, 3)
    with pytest.raises(ValueError, match="up to 1024"):
        ops.layernorm_rows_nchw(z(1, 2048), z(2048, dt=torch.float32), z(2048, dt=torch.float32), 1e-6, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------------ backbones
def _net(geo, sd):
    from anyedit_amd.checkpoints import load_uniformer
    from anyedit_amd.uniformer import UniFormer
    net = UniFormer(layers=list(geo["layers"]), embed_dim=list(geo["embed_dim"]), head_dim=geo["head_dim"])
    load_uniformer(net, sd)
    return net.to(DEV)


@pytest.fixture(scope="module")
def tiny():
    sd = sub_sd(load_golden("uniformer_tiny_w"), "w.")
    return _net(R.TINY, sd), sd, load_golden("uniformer_tiny_io")


def _judge_levels(label, hip, ctl, ref):
    report, ok = [], True
    for level in range(4):
        assert tuple(hip[level].shape) == tuple(ref[level].shape) and hip[level].dtype == torch.float32
        e_hip, e_ctl = rel_l2(hip[level].cpu(), ref[level]), rel_l2(ctl[level], ref[level])
        report.append(f"{label} level {level + 1} {tuple(ref[level].shape)}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
        ok &= e_hip <= 1.5 * e_ctl
    print("\n".join(report))
    assert ok, "\n".join(report)


@pytest.mark.parametrize("B,H,W", R.TINY_SIZES)
def test_tiny_backbone_vs_golden(tiny, B, H, W):
    net, sd, io = tiny
    name = f"{B}x{H}x{W}"
    x = T(io["x." + name])
    ref = [T(io[f"out.{name}.{k}"]) for k in range(4)]
    hip = net(x.to(DEV))
    assert isinstance(hip, tuple) and len(hip) == 4
    _judge_levels(name, hip, R.control(sd, x, R.TINY["head_dim"]), ref)
    # forward_rows: the same outputs as bf16 rows (ae_layernorm_bf16 there, ae_layernorm_rows_nchw here: one bf16 ulp, 2^-7 relative, plus the
    # fp32 differences of two kernels that compute the same normalisation); forward_both: one launch writes both, the rows are the rounded map
    rows = net.forward_rows(x.to(DEV))
    maps, rows2 = net.forward_both(x.to(DEV))
    for level, ((r, h, w), (r2, h2, w2)) in enumerate(zip(rows, rows2)):
        m = hip[level]
        assert (h, w) == (h2, w2) == tuple(m.shape[2:]) and r.dtype == BF and tuple(r.shape) == (B * h * w, m.shape[1])
        as_rows = m.permute(0, 2, 3, 1).reshape(B * h * w, -1)
        assert torch.equal(maps[level], m)
        assert torch.equal(_bits(r2), _bits(as_rows.to(BF)))
        assert bool(((r.float() - as_rows).abs() <= 2.0 ** -7 * as_rows.abs() + 1e-5).all())


def test_uniformer_s_width_vs_restatement():
    """The real widths (64, 128, 320, 512) and head dim 64 with layers (1, 1, 2, 1), one 96x64 image, seeded weights, against the fp32 restatement
    on the CPU."""
    geo = R.WIDE
    sd = R.seeded_state_dict(geo["layers"], geo["embed_dim"], geo["head_dim"], seed=1)
    x = R.smooth_pixels(1, 96, 64, seed=7)
    ref = R.forward(sd, x, geo["head_dim"])
    assert [tuple(r.shape) for r in ref] == [(1, 64, 24, 16), (1, 128, 12, 8), (1, 320, 6, 4), (1, 512, 3, 2)]
    _judge_levels("S width 96x64", _net(geo, sd)(x.to(DEV)), R.control(sd, x, geo["head_dim"]), ref)


def test_an_image_does_not_depend_on_its_batch(tiny):
    net, _, io = tiny
    x = T(io["x.2x64x48"]).to(DEV)
    both = net(x)
    one = net(x[1:2].clone())
    assert all(torch.equal(a[1:2], b) for a, b in zip(both, one)), "running an image with a neighbour changed its maps"
    assert not torch.equal(both[0][0], both[0][1])


def test_forward_is_capturable_and_follows_a_weight_change(tiny):
    net, sd, io = tiny
    static = T(io["x.1x72x56"]).to(DEV)
    first = [m.clone() for m in net(static)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream: the backbone only ever uses the current one
        out = net(static)
    new = R.smooth_pixels(1, 72, 56, seed=11).to(DEV)
    static.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [m.clone() for m in out]
    before, mem = torch.cuda.memory_stats(DEV)["allocation.all.allocated"], torch.cuda.memory_allocated(DEV)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before and torch.cuda.memory_allocated(DEV) == mem, "a replay allocated"
    eager = net(new)
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager)), "graph replay differs from the eager forward of the same image"
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert not torch.equal(replayed[0], first[0])
    # in-place changes of a BatchNorm buffer and of a depthwise weight: the next eager call repacks (refolds) and follows them
    for p in (net.blocks1[0].norm1.running_var, net.blocks2[0].attn.weight, net.blocks3[1].mlp.fc1.bias):
        keep = p.detach().clone()
        with torch.no_grad():
            p.mul_(1.5)
        changed = net(new)
        assert not torch.equal(changed[3], eager[3]), "an in-place weight change was not picked up"
        with torch.no_grad():
            p.copy_(keep)
        assert all(torch.equal(a, b) for a, b in zip(net(new), eager))


def test_load_uniformer_round_trip_through_a_file(tiny, tmp_path):
    net, sd, io = tiny
    path = str(tmp_path / "upernet_global_small.pth")
    torch.save({"state_dict": dict({"backbone." + k: v for k, v in sd.items()}, **{"decode_head.conv_seg.bias": torch.zeros(150)}), "meta": {}}, path)
    from anyedit_amd.uniformer import UniFormer
    other = UniFormer(layers=list(R.TINY["layers"]), embed_dim=list(R.TINY["embed_dim"]), head_dim=R.TINY["head_dim"], pretrained_path=path).to(DEV)
    x = T(io["x.1x40x104"]).to(DEV)
    assert all(torch.equal(a, b) for a, b in zip(other(x), net(x)))
