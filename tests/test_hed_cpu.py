"""CPU tests of the HED edge detector's host side: the restatement and the bf16-storage control against the reference's stored projections,
`checkpoints.load_hed`'s key handling, the refusal of images with a side below 16 pixels, the BGR flip of `HEDdetector.__call__`, the inputs of
the fuse kernel's GPU test, and the C ABI's declarations.  No GPU: nothing here launches a kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import hed_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return sub_sd(load_golden("hed_tiny_w"), "w."), load_golden("hed_tiny_io")


def _case(io, H, W):
    return io[f"image.{H}x{W}"], [T(io[f"proj.{H}x{W}.{k}"]) for k in range(5)]


def test_fixture_is_what_its_generator_describes(golden):
    sd, io = golden
    assert R.layers_of(sd) == R.TINY["layers"]
    assert tuple(sd[f"block{n}.convs.0.weight"].shape[0] for n in range(1, 6)) == R.TINY["channels"]
    assert torch.equal(sd["norm"].flatten(), torch.tensor(R.NORM))
    for i, (H, W) in enumerate(R.TINY_SIZES):
        img, sides = _case(io, H, W)
        assert img.dtype == np.uint8 and img.shape == (H, W, 3) and np.array_equal(img, R.smooth_image(H, W, seed=100 + i))
        assert [tuple(s.shape) for s in sides] == [(1, 1, H >> k, W >> k) for k in range(5)]
    H, W = R.TINY_SIZES[0]
    m = R.mean_logits(_case(io, H, W)[1], H, W)
    assert abs(float(m.mean())) < 1e-3 and abs(float(m.std()) - R.LOGIT_STD) < 1e-3, "the heads are rescaled on the first image"
    for name in ("hed_tiny_w", "hed_tiny_io"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 700 * 1024


@pytest.mark.parametrize("H,W", R.TINY_SIZES)
def test_restatement_matches_the_reference_to_fp32_rounding(golden, H, W):
    """The same torch operators in the same order as the reference: rel-L2 <= 1e-6 per projection (fp32 rounding; identical bits where the
    convolution picks the same algorithm), and the float64 network agrees with both to 1e-5."""
    sd, io = golden
    img, sides = _case(io, H, W)
    mine = R.forward(sd, R.to_nchw(img))
    mine64 = R.forward(sd, R.to_nchw(img), torch.float64)
    for k in range(5):
        assert tuple(mine[k].shape) == tuple(sides[k].shape)
        assert rel_l2(mine[k], sides[k]) <= 1e-6, k
        assert rel_l2(mine64[k].float(), sides[k]) <= 1e-5, k


@pytest.mark.parametrize("H,W", R.TINY_SIZES)
def test_control_stays_near_the_reference_and_the_edge_map_is_not_saturated(golden, H, W):
    """The bf16-storage control against the stored projections (figures printed: they are the yardstick of the GPU tests, not a gate; the bound
    here, 5e-2 on the mean logit map, only says the control is the same network), and the share of unsaturated pixels of the reference's map."""
    sd, io = golden
    img, sides = _case(io, H, W)
    ctl = R.control(sd, R.to_nchw(img))
    m_ref, m_ctl = R.mean_logits(sides, H, W), R.mean_logits(ctl, H, W)
    e_ref, e_ctl = R.edge_map(sides, H, W), R.edge_map(ctl, H, W)
    d = (e_ref.int() - e_ctl.int()).abs()
    share = float(((e_ref > 5) & (e_ref < 250)).float().mean())
    print(f"{H}x{W}: control rel-L2 per projection " + " ".join(f"{rel_l2(a, b):.2e}" for a, b in zip(ctl, sides))
          + f"; mean logit {rel_l2(m_ctl, m_ref):.2e}; uint8 map max diff {int(d.max())}, differing {100 * float((d > 0).float().mean()):.1f} %; "
          f"unsaturated {100 * share:.1f} %")
    assert 1e-4 < rel_l2(m_ctl, m_ref) < 5e-2
    assert share > 0.5
    assert e_ref.dtype == torch.uint8 and tuple(e_ref.shape) == (1, H, W)


def test_edge_map_is_the_detectors_arithmetic():
    """edge_map against the reference's lines :69-73 written out in numpy on already-resized maps (the resize is the identity at level 0)."""
    sides = [s for s in R.smooth_sides(2, 24, 20, seed=3)]
    m = R.mean_logits(sides, 24, 20)
    stack = np.stack([R.resize(s, 24, 20)[:, 0].numpy() for s in sides], axis=3)
    edge = 1 / (1 + np.exp(-np.mean(stack, axis=3).astype(np.float64)))
    edge = (edge * 255.0).clip(0, 255).astype(np.uint8)
    assert np.abs(np.mean(stack, axis=3) - m.numpy()).max() < 1e-5
    got = R.edge_map(sides, 24, 20).numpy().astype(int)
    assert np.abs(got - np.bitwise_not(edge).astype(int)).max() <= 1 and (got != np.bitwise_not(edge)).mean() < 0.01
    assert np.array_equal(R.edge_map(sides, 24, 20, invert=False).numpy(), 255 - R.edge_map(sides, 24, 20).numpy())


@pytest.mark.parametrize("H,W", [(16, 16), (17, 31), (50, 38), (33, 47)])
@pytest.mark.parametrize("B", [1, 2])
def test_fuse_test_inputs_are_unsaturated_and_rarely_near_an_integer(B, H, W):
    """What tests/test_hip_hed.py feeds the fuse kernel, checked where no GPU is needed: more than half of the reference's pixels in 5..250,
    and at most 1 % of them within 1e-3 of an integer before the truncation."""
    sides = R.smooth_sides(B, H, W, seed=H * 100 + W + B)
    v = R.edge_value(R.mean_logits([s.double() for s in sides], H, W))
    g = v.to(torch.uint8)
    near = float(((v - v.round()).abs() <= 1e-3).double().mean())
    print(f"B={B} {H}x{W}: in 5..250 {100 * float(((g >= 5) & (g <= 250)).double().mean()):.1f} %, within 1e-3 of an integer {100 * near:.2f} %")
    assert float(((g >= 5) & (g <= 250)).double().mean()) > 0.5 and near <= 0.01


# ------------------------------------------------------------------------------------------------------------ host code of the package
def _tiny_net():
    from anyedit_amd.hed import ControlNetHED_Apache2
    return ControlNetHED_Apache2(**R.TINY)


def test_model_keeps_the_reference_names_and_defaults(golden):
    from anyedit_amd.hed import ControlNetHED_Apache2
    sd, _ = golden
    net = _tiny_net()
    assert set(net.state_dict()) == set(sd)
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in net.state_dict().items())
    with torch.device("meta"):
        full = ControlNetHED_Apache2()
    want = R.seeded_state_dict()
    assert {k: tuple(v.shape) for k, v in full.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert full.channels == R.CHANNELS and full.layers == R.LAYERS
    with pytest.raises(ValueError, match="multiples of 8"):
        ControlNetHED_Apache2(channels=(12, 32, 64, 64, 64))


@pytest.mark.parametrize("prefix", ["", "module.", "netNetwork."])
def test_load_hed_accepts_the_prefixes_and_is_strict(golden, prefix, tmp_path):
    from anyedit_amd.checkpoints import load_hed
    sd, _ = golden
    net = _tiny_net()
    form = load_hed(net, {prefix + k: v for k, v in sd.items()})
    assert form == (prefix.rstrip(".") or "state_dict")
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    missing = {prefix + k: v for k, v in sd.items() if k != "block3.convs.1.bias"}
    with pytest.raises(RuntimeError, match="block3.convs.1.bias"):
        load_hed(_tiny_net(), missing)
    extra = dict({prefix + k: v for k, v in sd.items()}, **{prefix + "block6.projection.bias": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="block6.projection.bias"):
        load_hed(_tiny_net(), extra)
    mixed = dict(sd)
    mixed["module.norm"] = mixed.pop("norm")            # a prefix on some keys only is not a prefix
    with pytest.raises(RuntimeError, match="norm"):
        load_hed(_tiny_net(), mixed)
    if prefix == "":
        path = str(tmp_path / "ControlNetHED.pth")
        torch.save(sd, path)
        net2 = _tiny_net()
        assert load_hed(net2, path) == "state_dict" and torch.equal(net2.block5.projection.weight, sd["block5.projection.weight"])


def _cpu_detector(golden):
    from anyedit_amd.hed import HEDdetector
    return HEDdetector(golden[0], device="cpu", **R.TINY)


@pytest.mark.parametrize("H,W", [(15, 40), (40, 15), (8, 8)])
def test_images_with_a_side_below_16_are_refused(golden, H, W):
    det = _cpu_detector(golden)
    with pytest.raises(ValueError, match="below 16"):
        det.detect_array(np.zeros((H, W, 3), np.uint8))
    with pytest.raises(ValueError, match="below 16"):
        det.detect(torch.zeros(1, H, W, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="below 16"):
        det.netNetwork(torch.zeros(1, 3, H, W))
    with pytest.raises(TypeError):
        det.detect_array(np.zeros((32, 32, 3), np.float32))


def test_call_hands_the_network_bgr_and_writes_what_it_returns(golden, tmp_path):
    """`__call__` with the device part replaced by a recording stand-in: the array it hands to `detect_array` is the file's pixels with the
    channel axis reversed (cv2.imread's order), and the file it writes holds the returned map; `img2scribble` is the same call."""
    from PIL import Image
    from anyedit_amd.tools.tool import img2scribble
    det = _cpu_detector(golden)
    rgb = R.smooth_image(40, 28, seed=5)
    assert not np.array_equal(rgb, rgb[:, :, ::-1])
    src, dst, dst2 = (str(tmp_path / n) for n in ("in.png", "out.png", "out2.png"))
    Image.fromarray(rgb).save(src)
    seen = []
    edge = (np.arange(40 * 28) % 256).astype(np.uint8).reshape(40, 28)

    def stand_in(image):
        seen.append(np.array(image))
        return edge

    det.detect_array = stand_in
    det(src, dst)
    assert img2scribble(src, dst2, det) == dst2
    assert len(seen) == 2 and all(np.array_equal(s, rgb[:, :, ::-1]) for s in seen)
    for out in (dst, dst2):
        back = np.array(Image.open(out))
        assert back.dtype == np.uint8 and np.array_equal(back, edge)


def test_entry_points_are_declared_and_bound():
    from anyedit_amd import _lib
    header = open(os.path.join(ROOT, "include", "anyedit_hip.h")).read()
    for name in ("ae_hed_stem_bf16", "ae_relu_bf16", "ae_hed_tail_bf16", "ae_hed_fuse"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"
