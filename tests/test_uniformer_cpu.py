"""CPU tests of the UniFormer backbone's host side: the restatement (tests/uniformer_ref.py) against the reference's stored maps, the fixture
condition on the bf16-storage control, the BatchNorm fold and the patch column order in float64, the floors of odd maps, the module's names and
state-dict keys, checkpoints.load_uniformer on every layout, and the refusals.  No GPU: nothing here launches a kernel."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import uniformer_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = [f"{B}x{H}x{W}" for B, H, W in R.TINY_SIZES]


@pytest.fixture(scope="module")
def golden():
    return sub_sd(load_golden("uniformer_tiny_w"), "w."), load_golden("uniformer_tiny_io")


def test_fixture_is_what_its_generator_describes(golden):
    sd, io = golden
    want = R.seeded_state_dict(R.TINY["layers"], R.TINY["embed_dim"], R.TINY["head_dim"], seed=R.TINY_SEED)
    assert set(sd) == set(want)
    assert all(torch.equal(sd[k], want[k]) for k in want), "the stored weights are not seeded_state_dict(TINY_SEED)"
    assert R.layers_of(sd) == R.TINY["layers"]
    for i, (name, (B, H, W)) in enumerate(zip(NAMES, R.TINY_SIZES)):
        assert torch.equal(T(io["x." + name]), R.smooth_pixels(B, H, W, seed=200 + i))
        h, w = H // 4, W // 4
        for level, C in enumerate(R.TINY["embed_dim"]):
            assert io[f"out.{name}.{level}"].shape == (B, C, h, w) and io[f"out.{name}.{level}"].dtype.name == "float32"
            h, w = h // 2, w // 2
    assert [io[f"out.1x72x56.{k}"].shape[2:] for k in range(4)] == [(18, 14), (9, 7), (4, 3), (2, 1)], "both floors occur"
    bn = [k for k in sd if k.endswith("running_var")]
    assert len(bn) == 4
    for k in bn:
        q = k[:-len("running_var")]
        assert 0.5 <= float(sd[k].min()) and float(sd[k].max()) <= 2.0 and float(sd[k].max() / sd[k].min()) > 2.0
        assert float(sd[q + "running_mean"].abs().mean()) > 0.1 and float((sd[q + "weight"] - 1).abs().mean()) > 0.1
        assert float(sd[q + "bias"].abs().mean()) > 0.05
    for f in ("uniformer_tiny_w.npz", "uniformer_tiny_io.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference_to_fp32_rounding(golden, name):
    sd, io = golden
    outs = R.forward(sd, T(io["x." + name]), R.TINY["head_dim"])
    for level, o in enumerate(outs):
        ref = T(io[f"out.{name}.{level}"])
        assert o.dtype == torch.float32 and tuple(o.shape) == tuple(ref.shape)
        assert rel_l2(o, ref) <= 1e-5, (name, level, rel_l2(o, ref))


@pytest.mark.parametrize("name", NAMES)
def test_control_meets_the_fixture_condition(golden, name):
    sd, io = golden
    lo, hi = R.FIXTURE_BAND
    for level, c in enumerate(R.control(sd, T(io["x." + name]), R.TINY["head_dim"])):
        e = rel_l2(c, T(io[f"out.{name}.{level}"]))
        assert lo <= e <= hi, (name, level, e)


def _bn_case(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    return dict(weight=r(N, K, 1, 1), bias=r(N), gamma=0.5 + torch.rand(K, generator=g, dtype=F64), beta=r(K), mean=r(K),
                var=0.5 + 1.5 * torch.rand(K, generator=g, dtype=F64))


@pytest.mark.parametrize("which", ["module", "restatement"])
@pytest.mark.parametrize("N,K", [(16, 16), (64, 16), (40, 24)])
def test_bn_fold_equals_bn_then_convolution_in_float64(N, K, which):
    """conv(BN(x)) = (W s) x + (W t + b): the folded weight and bias applied to x against F.batch_norm then F.conv2d, float64, 1e-12 relative"""
    if which == "module":
        from anyedit_amd.uniformer import fold_bn
    else:
        fold_bn = R.fold_bn
    c = _bn_case(N, K, seed=N + K)
    x = torch.randn(2, K, 5, 3, generator=torch.Generator().manual_seed(1), dtype=F64) * 2.0 + 0.5
    want = F.conv2d(F.batch_norm(x, c["mean"], c["var"], c["gamma"], c["beta"], False, 0.0, 1e-5), c["weight"], c["bias"])
    w, b = fold_bn(c["weight"], c["bias"], c["gamma"], c["beta"], c["mean"], c["var"], 1e-5)
    assert w.dtype == F64 and tuple(w.shape) == (N, K) and tuple(b.shape) == (N,)
    got = F.conv2d(x, w.view(N, K, 1, 1), b)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12
    for drop in ("gamma", "beta", "mean", "var"):          # the data can tell: a fold without one of the four is far away
        d = dict(c)
        d[drop] = torch.ones(K, dtype=F64) if drop in ("gamma", "var") else torch.zeros(K, dtype=F64)
        w2, b2 = fold_bn(d["weight"], d["bias"], d["gamma"], d["beta"], d["mean"], d["var"], 1e-5)
        assert float((F.conv2d(x, w2.view(N, K, 1, 1), b2) - want).abs().max() / want.abs().max()) > 1e-2, drop


def _patch2_rows(x):
    """the gather ae_patch2_rows_bf16 is declared to do, on [B, H, W, C]: column (2 ky + kx) C + c, floor"""
    B, H, W, C = x.shape
    h, w = H // 2, W // 2
    x = x[:, :2 * h, :2 * w].reshape(B, h, 2, w, 2, C).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(B * h * w, 4 * C)


@pytest.mark.parametrize("H,W", [(4, 6), (5, 7), (9, 4)])
def test_pack_patch2_column_order_against_conv2d(H, W):
    from anyedit_amd import ops
    g = torch.Generator().manual_seed(H * 10 + W)
    B, Cin, Cout = 2, 8, 12
    w = torch.randn(Cout, Cin, 2, 2, generator=g).bfloat16().float()
    x = torch.randn(B, Cin, H, W, generator=g, dtype=F64)
    want = F.conv2d(x, w.to(F64), stride=2).permute(0, 2, 3, 1).reshape(-1, Cout)
    wp = ops.pack_patch2(w)
    assert wp.dtype == torch.bfloat16 and tuple(wp.shape) == (Cout, 4 * Cin)
    got = _patch2_rows(x.permute(0, 2, 3, 1)) @ wp.to(F64).t()
    assert want.shape[0] == B * (H // 2) * (W // 2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_pack_dwconv_is_tap_major_fp32():
    from anyedit_amd import ops
    for k in (3, 5):
        w = torch.randn(24, 1, k, k, generator=torch.Generator().manual_seed(k))
        p = ops.pack_dwconv(w)
        assert p.dtype == torch.float32 and tuple(p.shape) == (k * k, 24) and p.is_contiguous()
        assert all(torch.equal(p[ky * k + kx], w[:, 0, ky, kx]) for ky in range(k) for kx in range(k))
    with pytest.raises(ValueError, match="depthwise"):
        ops.pack_dwconv(torch.zeros(8, 1, 7, 7))
    with pytest.raises(ValueError, match="depthwise"):
        ops.pack_dwconv(torch.zeros(8, 2, 3, 3))


@pytest.mark.parametrize("H,W", [(72, 56), (33, 47), (63, 32)])
def test_odd_maps_floor(golden, H, W):
    """every stage's size is the floor of the previous one's half (a quarter for the first): the convolution drops the last row / column, and the
    dropped pixels do not reach the outputs"""
    sd, _ = golden
    x = R.smooth_pixels(1, H, W, seed=3)
    outs = R.forward(sd, x, R.TINY["head_dim"])
    h, w = H // 4, W // 4
    for o in outs:
        assert tuple(o.shape[2:]) == (h, w)
        h, w = h // 2, w // 2
    h4, w4 = H // 4 * 4, W // 4 * 4
    if (h4, w4) != (H, W):
        cropped = R.forward(sd, x[:, :, :h4, :w4].contiguous(), R.TINY["head_dim"])
        assert all(torch.equal(a, b) for a, b in zip(outs, cropped))


# ------------------------------------------------------------------------------------------------------------ host code of the package
def _tiny_net():
    from anyedit_amd.uniformer import UniFormer
    return UniFormer(**{k: list(v) if isinstance(v, tuple) else v for k, v in R.TINY.items()})


def test_model_keeps_the_reference_names_and_defaults(golden):
    import inspect
    from anyedit_amd import uniformer as U
    sd, _ = golden
    net = _tiny_net()
    assert set(net.state_dict()) == set(sd)
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in net.state_dict().items())
    assert not net.training
    with torch.device("meta"):
        full = U.UniFormer()
    want = R.seeded_state_dict(**R.S_GEOMETRY)
    assert {k: tuple(v.shape) for k, v in full.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert [len(getattr(full, f"blocks{n}")) for n in range(1, 5)] == [3, 4, 8, 3]
    assert [b.attn.num_heads for b in full.blocks3] == [5] * 8 and [b.attn.num_heads for b in full.blocks4] == [8] * 3
    assert full.blocks3[0].attn.scale == 64 ** -0.5
    assert full.patch_embed1.norm.eps == 1e-5 and full.blocks3[0].norm1.eps == 1e-6 and full.norm4.eps == 1e-6
    assert list(inspect.signature(U.UniFormer.__init__).parameters)[1:] == [
        "layers", "img_size", "in_chans", "num_classes", "embed_dim", "head_dim", "mlp_ratio", "qkv_bias", "qk_scale", "representation_size", "drop_rate",
        "attn_drop_rate", "drop_path_rate", "norm_layer", "pretrained_path", "use_checkpoint", "checkpoint_num", "windows", "hybrid", "window_size"]
    for name in ("Mlp", "CMlp", "CBlock", "Attention", "SABlock", "PatchEmbed", "UniFormer"):
        assert inspect.isclass(getattr(U, name))


@pytest.mark.parametrize("layout", ["bare", "backbone.", "module.backbone.", "state_dict", "module."])
def test_load_uniformer_accepts_the_layouts_and_is_strict(golden, layout, tmp_path):
    from anyedit_amd.checkpoints import load_uniformer
    sd, _ = golden
    heads = {"decode_head.conv_seg.weight": torch.zeros(3, 4, 1, 1), "auxiliary_head.conv_seg.bias": torch.zeros(3)}
    if layout == "bare":
        wrap = lambda d: dict(d)
    elif layout == "module.":
        wrap = lambda d: {"module." + k: v for k, v in d.items()}
    elif layout == "state_dict":
        wrap = lambda d: {"state_dict": dict({"backbone." + k: v for k, v in d.items()}, **heads), "meta": {"epoch": 1}}
    else:
        pref = layout
        wrap = lambda d: dict({pref + k: v for k, v in d.items()}, **{pref[:-len("backbone.")] + k: v for k, v in heads.items()})
    net = _tiny_net()
    load_uniformer(net, wrap(sd))
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    missing = {k: v for k, v in sd.items() if k != "blocks2.0.norm1.running_var"}
    with pytest.raises(RuntimeError, match="blocks2.0.norm1.running_var"):
        load_uniformer(_tiny_net(), wrap(missing))
    extra = dict(sd, **{"blocks5.0.pos_embed.bias": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="blocks5.0.pos_embed.bias"):
        load_uniformer(_tiny_net(), wrap(extra))
    path = str(tmp_path / "upernet.pth")
    torch.save(wrap(sd), path)
    net2 = _tiny_net()
    load_uniformer(net2, path)
    assert all(torch.equal(v, sd[k]) for k, v in net2.state_dict().items())


def test_load_uniformer_refuses_a_segmentor_with_unknown_parts(golden):
    from anyedit_amd.checkpoints import load_uniformer
    sd, _ = golden
    with pytest.raises(KeyError, match="neck"):
        load_uniformer(_tiny_net(), dict({"backbone." + k: v for k, v in sd.items()}, **{"neck.weight": torch.zeros(1)}))


def test_what_is_not_built_is_refused_with_a_sentence():
    from anyedit_amd.uniformer import UniFormer, CBlock
    small = dict(layers=[1, 1, 1, 1], embed_dim=[8, 8, 32, 32], head_dim=32)
    for kw, word in ((dict(windows=True), "windows=True"), (dict(hybrid=True), "hybrid=True"), (dict(representation_size=64), "representation_size"),
                     (dict(use_checkpoint=True), "use_checkpoint")):
        with pytest.raises(NotImplementedError, match=word + ".*not built"):
            UniFormer(**small, **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        CBlock(dim=12, num_heads=1)
    with pytest.raises(ValueError, match="heads"):
        UniFormer(layers=[1, 1, 1, 1], embed_dim=[8, 8, 40, 64], head_dim=32)
    with pytest.raises(NotImplementedError, match="training"):
        UniFormer(**small).train()


@pytest.mark.parametrize("H,W", [(31, 64), (64, 31), (16, 16)])
def test_images_with_a_side_below_32_are_refused(H, W):
    net = _tiny_net()
    with pytest.raises(ValueError, match="below 32"):
        net(torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="below 32"):
        net.forward_rows(torch.zeros(1, 3, H, W))
    with pytest.raises(TypeError):
        net(torch.zeros(1, 3, 64, 64, dtype=torch.float64))


def test_entry_points_are_declared_and_bound():
    from anyedit_amd import _lib
    header = open(os.path.join(ROOT, "include", "anyedit_hip.h")).read()
    for name in ("ae_dwconv_rows_bf16", "ae_patch2_rows_bf16", "ae_layernorm_rows_nchw"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"
