"""CPU tests of the UPerNet head's host side: the restatement (tests/upernet_ref.py) against the reference's stored logits and labels, the fixture
conditions on the bf16-storage control, the BatchNorm fold in float64, the bin and tap arithmetic of the kernels against torch's operators,
`rescale_size`, the palette fixture, the red / blue exchange of the file `img2seg` writes, the module's state-dict keys,
checkpoints.load_segmentor on every layout, and the refusals.  No GPU: nothing here launches a kernel."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SIZES = {f"{B}x{H}x{W}": (B, H, W) for B, H, W in UR.TINY_SIZES}
NAMES = list(SIZES)


@pytest.fixture(scope="module")
def golden():
    return sub_sd(load_golden("upernet_tiny_w"), "w."), load_golden("upernet_tiny_io"), load_golden("uniformer_tiny_io")


def _maps(bio, name):
    return [T(bio[f"out.{name}.{k}"]) for k in range(4)]


def _oris(name):
    _, H, W = SIZES[name]
    return [(H, W), R.SECOND_ORI[name]]


def test_fixture_is_what_its_generator_describes(golden):
    sd, io, bio = golden
    want = R.seeded_head_state_dict(seed=R.TINY_SEED, **R.TINY_HEAD)
    assert set(sd) == set(want)
    assert all(torch.equal(sd[k], want[k]) for k in want), "the stored weights are not seeded_head_state_dict(TINY_SEED)"
    assert bio["out.1x72x56.3"].shape[2:] == (2, 1), "the pools of 3 and 6 repeat pixels on this map"
    bn = [k for k in sd if k.endswith("running_var")]
    assert len(bn) == 4 + 1 + 3 + 3 + 1
    for k in bn:
        q = k[:-len("running_var")]
        assert 0.5 <= float(sd[k].min()) and float(sd[k].max()) <= 2.0 and float(sd[k].max() / sd[k].min()) > 2.0
        assert float(sd[q + "running_mean"].abs().mean()) > 0.1 and float((sd[q + "weight"] - 1).abs().mean()) > 0.1
        assert float(sd[q + "bias"].abs().mean()) > 0.05
    for name, (B, H, W) in SIZES.items():
        assert io["logits." + name].shape == (B, 150, H // 4, W // 4) and io["logits." + name].dtype.name == "float32"
        for Ho, Wo in _oris(name):
            lab = io[f"labels.{name}.{Ho}x{Wo}"]
            assert lab.shape == (B, Ho, Wo) and lab.dtype.name == "uint8"
        assert (R.SECOND_ORI[name][0] % (H // 4) or R.SECOND_ORI[name][1] % (W // 4)) and R.SECOND_ORI[name] != (H, W)
    for f in ("upernet_tiny_w.npz", "upernet_tiny_io.npz", "ade_palette.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference(golden, name):
    sd, io, bio = golden
    _, H, W = SIZES[name]
    logits = R.head_forward(sd, _maps(bio, name), R.TINY_HEAD["pool_scales"])
    ref = T(io["logits." + name])
    assert logits.dtype == torch.float32 and tuple(logits.shape) == tuple(ref.shape)
    assert rel_l2(logits, ref) <= 1e-5, rel_l2(logits, ref)
    for Ho, Wo in _oris(name):
        key = f"{name}.{Ho}x{Wo}"
        labels, margin = T(io["labels." + key]).long(), T(io["margin." + key])
        clear = margin > 1e-4
        assert float((~clear).float().mean()) < 0.005, "fewer than 0.5 % of the pixels are excluded"
        mine = R.segment(logits, (H, W), (Ho, Wo))
        assert torch.equal(mine[clear], labels[clear]), key
        assert torch.equal(R.top_two_margin(R.resize_twice(ref, (H, W), (Ho, Wo))), margin), "the stored margins are those of the stored logits"


@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(golden, name):
    sd, io, bio = golden
    _, H, W = SIZES[name]
    ref = T(io["logits." + name])
    ctl = R.head_control(sd, _maps(bio, name), R.TINY_HEAD["pool_scales"])
    lo, hi = UR.FIXTURE_BAND
    e = rel_l2(ctl, ref)
    assert lo <= e <= hi, (name, e)
    for Ho, Wo in _oris(name):
        key = f"{name}.{Ho}x{Wo}"
        full = R.resize_twice(ref, (H, W), (Ho, Wo))
        e_abs = float((R.resize_twice(ctl, (H, W), (Ho, Wo)) - full).abs().max())
        near = float((T(io["margin." + key]) < 3 * e_abs).float().mean())
        distinct = len(np.unique(io["labels." + key]))
        flips = int((full.softmax(1).argmax(1) != full.argmax(1)).sum())
        print(f"{key}: control rel-L2 {e:.2e}, e_ctl {e_abs:.2e}, {100 * near:.1f} % within 3 e_ctl, {distinct} labels, {flips} softmax flips")
        assert distinct >= R.MIN_DISTINCT and near <= R.NEAR_SHARE
        assert flips == int(io["softmax_flips." + key]), "the count of pixels the softmax's rounding relabels, as recorded"


def _bn_case(N, K, k, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    return dict(weight=r(N, K, k, k), gamma=0.5 + torch.rand(N, generator=g, dtype=F64), beta=r(N), mean=r(N), var=0.5 + 1.5 * torch.rand(N, generator=g, dtype=F64))


@pytest.mark.parametrize("which", ["ops", "restatement"])
@pytest.mark.parametrize("N,K,k", [(16, 16, 1), (32, 24, 3), (8, 40, 3)])
def test_bn_fold_equals_convolution_then_bn_in_float64(N, K, k, which):
    """BN(conv(x)) = conv(x, W s) + (beta - mean s): the folded pair against F.conv2d then F.batch_norm, float64, 1e-12 relative; a fold that drops
    any one of the four vectors is off by more than 1e-2"""
    if which == "ops":
        from anyedit_amd.ops import fold_bn_after_conv as fold
    else:
        fold = R.fold_bn_after_conv
    c = _bn_case(N, K, k, seed=N + K)
    x = torch.randn(2, K, 5, 4, dtype=F64, generator=torch.Generator().manual_seed(3))
    want = F.batch_norm(F.conv2d(x, c["weight"], None, padding=k // 2), c["mean"], c["var"], c["gamma"], c["beta"], False, 0.0, R.BN_EPS)
    w, b = fold(c["weight"], c["gamma"], c["beta"], c["mean"], c["var"], R.BN_EPS)
    assert tuple(w.shape) == tuple(c["weight"].shape) and tuple(b.shape) == (N,)
    scale = float(want.abs().max())
    assert float((F.conv2d(x, w, b, padding=k // 2) - want).abs().max()) <= 1e-12 * scale
    neutral = dict(gamma=torch.ones(N, dtype=F64), beta=torch.zeros(N, dtype=F64), mean=torch.zeros(N, dtype=F64), var=torch.ones(N, dtype=F64) - R.BN_EPS)
    for dropped in neutral:
        w2, b2 = fold(**{**c, dropped: neutral[dropped]}, eps=R.BN_EPS)
        assert float((F.conv2d(x, w2, b2, padding=k // 2) - want).abs().max()) > 1e-2 * scale, dropped


@pytest.mark.parametrize("H,W", [(1, 1), (2, 1), (4, 3), (7, 5), (6, 6), (16, 16), (3, 11)])
def test_bin_arithmetic_is_adaptive_avg_pool(H, W):
    x = torch.randn(2, H, W, 8, dtype=F64, generator=torch.Generator().manual_seed(H * 20 + W))
    scales = (1, 2, 3, 6, 8)
    got = R.pool_rows64(x, scales)
    want = torch.cat([F.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), s).permute(0, 2, 3, 1).reshape(2, s * s, 8) for s in scales], 1)
    assert tuple(got.shape) == (2, sum(s * s for s in scales), 8)
    assert float((got - want).abs().max()) < 1e-13
    for n in (1, 2, 5, 16):
        for s in scales:
            bins = R.pool_bins(n, s)
            assert bins[0][0] == 0 and bins[-1][1] == n and all(0 <= a < b <= n for a, b in bins)
            if n < s:
                assert sum(b - a for a, b in bins) > n, "bins repeat pixels when n < s"


PAIRS = [((1, 1), (3, 2)), ((2, 1), (4, 3)), ((6, 6), (16, 16)), ((4, 3), (18, 14)), ((9, 7), (18, 14)), ((7, 9), (3, 4)), ((5, 7), (5, 7)), ((18, 14), (72, 56)),
         ((10, 26), (40, 104))]


@pytest.mark.parametrize("src,dst", PAIRS)
def test_tap_arithmetic_is_interpolate(src, dst):
    (h, w), (H, W) = src, dst
    x = torch.randn(2, h, w, 8, dtype=F64, generator=torch.Generator().manual_seed(h * 100 + W))
    want = F.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    got, mags = R.bilinear64(x, H, W)
    assert float((got - want).abs().max()) < 1e-12
    if src == dst:
        assert torch.equal(got, x)
    i0, i1, l1 = R.axis_taps(h, H)
    assert int(i0.min()) >= 0 and int(i1.max()) <= h - 1 and float(l1.min()) >= 0 and float(l1.max()) < 1


@pytest.mark.parametrize("src,mid,out", [((1, 1), (4, 4), (4, 4)), ((18, 14), (72, 56), (101, 83)), ((10, 26), (40, 104), (23, 57)), ((3, 2), (12, 8), (12, 8))])
def test_tap_arithmetic_composed_twice(src, mid, out):
    x = torch.randn(1, *src, 8, dtype=F64, generator=torch.Generator().manual_seed(sum(out)))
    want = R.resize_twice(x.permute(0, 3, 1, 2), mid, out).permute(0, 2, 3, 1)
    got = R.bilinear64(R.bilinear64(x, *mid)[0], *out)[0]
    assert float((got - want).abs().max()) < 1e-12


def test_rescale_size_matches_the_stored_table(golden):
    from anyedit_amd.uniformer import upernet
    table = golden[1]["rescale.table"]
    assert len(table) >= 10
    for w, h, nw, nh in table.tolist():
        assert R.rescale_size((w, h), (2048, 512)) == (nw, nh), (w, h)
        assert upernet.rescale_size((w, h), upernet.IMG_SCALE) == (nw, nh), (w, h)
    assert R.rescale_size((512, 512), (2048, 512)) == (512, 512), "the size AnyEdit loads is not resized"


def test_palette_fixture():
    pal = load_golden("ade_palette")
    p = pal["palette"]
    assert p.shape == (150, 3) and p.dtype.name == "uint8"
    assert p[:3].tolist() == [[120, 120, 120], [180, 120, 120], [6, 230, 230]]
    assert len(pal["classes"]) == 150 and str(pal["classes"][0]) == "wall"
    assert len({tuple(r) for r in p.tolist()}) > 140, "the colours tell the classes apart"


def test_stored_colour_image_is_palette_of_label(golden):
    io, p = golden[1], load_golden("ade_palette")["palette"]
    for name, (B, H, W) in SIZES.items():
        assert np.array_equal(io["colour." + name], p[io[f"labels.{name}.{H}x{W}"][0]])


class _FakeSegmentor:
    def __init__(self, colours):
        self.colours, self.seen = colours, None

    def colour_image(self, bgr):
        self.seen = bgr
        return self.colours


def test_img2seg_writes_red_and_blue_exchanged(tmp_path):
    """img2seg hands the network BGR and saves colour_image(...)[..., ::-1]: the file's pixels are the palette's with red and blue exchanged"""
    from PIL import Image
    from anyedit_amd.tools.tool import img2seg
    g = np.random.default_rng(0)
    rgb = g.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    colours = g.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(rgb).save(src)
    fake = _FakeSegmentor(colours)
    assert img2seg(src, dst, fake) == dst
    assert np.array_equal(fake.seen, rgb[:, :, ::-1]), "the network is handed BGR, as cv2.imread yields it"
    written = np.array(Image.open(dst).convert("RGB"))
    assert np.array_equal(written[..., 0], colours[..., 2]) and np.array_equal(written[..., 2], colours[..., 0]) and np.array_equal(written[..., 1], colours[..., 1])


# ------------------------------------------------------------------------------------------------ module, loader, refusals
def _tiny_model(**kw):
    from anyedit_amd.uniformer import UniFormer
    from anyedit_amd.uniformer.upernet import EncoderDecoder, UPerHead
    geo, hg = UR.TINY, R.TINY_HEAD
    backbone = UniFormer(layers=list(geo["layers"]), embed_dim=list(geo["embed_dim"]), head_dim=geo["head_dim"])
    head = UPerHead(pool_scales=hg["pool_scales"], in_channels=list(hg["in_channels"]), channels=hg["channels"], num_classes=hg["num_classes"],
                    norm_cfg=dict(type="BN", requires_grad=True), in_index=[0, 1, 2, 3], dropout_ratio=0.1, align_corners=False)
    return EncoderDecoder(backbone, head, test_cfg=dict(mode="whole"), **kw)


def _full_sd(golden):
    bsd = sub_sd(load_golden("uniformer_tiny_w"), "w.")
    return dict({"backbone." + k: v for k, v in bsd.items()}, **{"decode_head." + k: v for k, v in golden[0].items()})


def test_module_has_the_reference_state_dict_keys(golden):
    model = _tiny_model()
    keys = set(model.state_dict())
    assert keys == set(_full_sd(golden))
    for k in ("decode_head.psp_modules.0.1.conv.weight", "decode_head.lateral_convs.1.bn.running_var", "decode_head.conv_seg.bias",
              "decode_head.fpn_bottleneck.bn.num_batches_tracked", "decode_head.bottleneck.conv.weight", "decode_head.fpn_convs.2.bn.weight"):
        assert k in keys, k
    assert tuple(model.decode_head.bottleneck.conv.weight.shape) == (32, 64 + 4 * 32, 3, 3)


def test_load_segmentor_layouts(golden, tmp_path):
    from anyedit_amd.checkpoints import load_segmentor
    sd = _full_sd(golden)
    pal = load_golden("ade_palette")
    meta = {"CLASSES": [str(c) for c in pal["classes"]], "PALETTE": pal["palette"].tolist()}
    model = _tiny_model()
    assert load_segmentor(model, {"state_dict": sd, "meta": meta}) == "state_dict"
    assert torch.equal(model.decode_head.conv_seg.bias, sd["decode_head.conv_seg.bias"])
    assert np.array_equal(model.PALETTE, pal["palette"]) and model.PALETTE.dtype == np.uint8 and model.CLASSES[0] == "wall"
    aux = dict(sd, **{"auxiliary_head.conv_seg.weight": torch.zeros(150, 8, 1, 1), "auxiliary_head.convs.0.bn.running_mean": torch.zeros(8)})
    assert load_segmentor(_tiny_model(), aux) == "state_dict-auxiliary_head"
    assert load_segmentor(_tiny_model(), {"state_dict": {"module." + k: v for k, v in aux.items()}}) == "module-auxiliary_head"
    missing = {k: v for k, v in sd.items() if k != "decode_head.fpn_convs.1.bn.running_var"}
    with pytest.raises(RuntimeError, match="decode_head.fpn_convs.1.bn.running_var"):
        load_segmentor(_tiny_model(), missing)
    with pytest.raises(RuntimeError, match="decode_head.extra.weight"):
        load_segmentor(_tiny_model(), dict(sd, **{"decode_head.extra.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="neck.weight"):
        load_segmentor(_tiny_model(), dict(sd, **{"neck.weight": torch.zeros(1)}))
    # a palette= argument overrides the checkpoint's
    other = pal["palette"][::-1].copy()
    over = _tiny_model(palette=other)
    load_segmentor(over, {"state_dict": sd, "meta": meta})
    assert np.array_equal(over.PALETTE, other)
    # through a file
    path = str(tmp_path / "upernet_global_small.pth")
    torch.save({"state_dict": aux, "meta": meta}, path)
    filed = _tiny_model(pretrained=path)
    assert np.array_equal(filed.PALETTE, pal["palette"]) and torch.equal(filed.backbone.norm4.weight, sd["backbone.norm4.weight"])
    with pytest.raises(ValueError, match="150 rows"):
        _tiny_model(palette=pal["palette"][:10])


def test_refusals():
    from anyedit_amd.uniformer import UniFormer
    from anyedit_amd.uniformer.upernet import ConvModule, EncoderDecoder, UPerHead
    hg = dict(pool_scales=(1, 2, 3, 6), in_channels=[16, 32, 64, 64], channels=32, norm_cfg=dict(type="BN"))
    with pytest.raises(NotImplementedError, match="align_corners=True"):
        UPerHead(num_classes=150, align_corners=True, **hg)
    with pytest.raises(NotImplementedError, match="at most 256 classes"):
        UPerHead(num_classes=257, **hg)
    with pytest.raises(NotImplementedError, match="pool_scales"):
        UPerHead(num_classes=150, **dict(hg, pool_scales=(1, 2, 3, 6, 8)))
    with pytest.raises(NotImplementedError, match="pool_scales"):
        UPerHead(num_classes=150, **dict(hg, pool_scales=(1, 12)))
    with pytest.raises(NotImplementedError, match="norm_cfg"):
        UPerHead(num_classes=150, **dict(hg, norm_cfg=dict(type="GN", num_groups=8)))
    with pytest.raises(NotImplementedError, match="kernel 5"):
        ConvModule(8, 8, 5, padding=2)
    with pytest.raises(ValueError, match="multiples of 8"):
        ConvModule(12, 8, 1)
    head = UPerHead(num_classes=150, **hg)
    with pytest.raises(NotImplementedError, match="training mode"):
        head.train()
    geo = UR.TINY
    backbone = UniFormer(layers=list(geo["layers"]), embed_dim=list(geo["embed_dim"]), head_dim=geo["head_dim"])
    with pytest.raises(NotImplementedError, match="mode='slide'"):
        EncoderDecoder(backbone, head, test_cfg=dict(mode="slide", crop_size=(512, 512), stride=(341, 341)))
    with pytest.raises(NotImplementedError, match="neck"):
        EncoderDecoder(backbone, head, neck=dict(type="FPN"))
    model = EncoderDecoder(backbone, head, test_cfg=dict(mode="whole"))
    with pytest.raises(NotImplementedError, match="training mode"):
        model.train()
    with pytest.raises(NotImplementedError, match="aug_test"):
        model.aug_test([None], [None])
    with pytest.raises(NotImplementedError, match="slide"):
        model.slide_inference(None, None, True)
    with pytest.raises(NotImplementedError, match="flipped"):
        model.simple_test(torch.zeros(1, 3, 32, 32), flip=True)
    with pytest.raises(TypeError, match="uint8 BGR"):
        model.preprocess(np.zeros((8, 8, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="no palette"):
        model._palette_on("cpu")


def test_preprocess_of_a_512_image_is_exact():
    """a 512x512 image is not resized: the pixels are the BGR -> RGB flip and the normalisation, nothing else"""
    model = _tiny_model()
    bgr = np.random.default_rng(1).integers(0, 256, (512, 512, 3), dtype=np.uint8)
    x, ori = model.preprocess(bgr, device="cpu")
    from anyedit_amd.uniformer.upernet import IMG_MEAN, IMG_STD
    want = (torch.from_numpy(bgr[:, :, ::-1].copy()).permute(2, 0, 1).float() - torch.tensor(IMG_MEAN).view(3, 1, 1)) / torch.tensor(IMG_STD).view(3, 1, 1)
    assert ori == (512, 512) and torch.equal(x[0], want)
    x2, ori2 = model.preprocess(np.zeros((300, 400, 3), dtype=np.uint8), device="cpu")
    assert ori2 == (300, 400) and tuple(x2.shape) == (1, 3, 512, 683)
