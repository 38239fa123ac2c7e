"""CPU tests of Depth Anything V2's host side: the restatement and the bf16-storage control against the reference's stored depths, `get_size` against
the reference's recorded results, `checkpoints.load_depth_anything`'s key handling, the refusals, the colour table against matplotlib, the index
arithmetic against the recorded result, and the C ABI's declarations.  No GPU: nothing here launches a kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import dpt_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = R.TINY_TOWER["num_heads"]


@pytest.fixture(scope="module")
def golden():
    return sub_sd(load_golden("dpt_tiny_w"), "w."), load_golden("dpt_tiny_io")


def _tiny_model():
    from anyedit_amd.depth_anything_v2 import DepthAnythingV2
    return DepthAnythingV2(config=R.TINY_TOWER, **R.TINY)


def test_fixture_is_what_its_generator_describes(golden):
    """The stored weights are the seeded ones up to the rescaled last layer, the images are the generator's, and every stored depth meets the
    condition the issue sets: clipped share in [2 %, 50 %], std / mean >= 0.25."""
    sd, io = golden
    want = R.seeded_state_dict(R.TINY_TOWER, R.TINY["features"], R.TINY["out_channels"], seed=R.TINY_SEED)
    assert set(sd) == set(want)
    for k, v in want.items():
        if "output_conv2.2." not in k:
            assert torch.equal(sd[k], v), k
    for i, (B, H, W) in enumerate(R.TINY_SIZES):
        px, d = T(io[f"pixels.{B}x{H}x{W}"]), T(io[f"depth.{B}x{H}x{W}"])
        assert torch.equal(px, R.smooth_pixels(B, H, W, seed=100 + i)) and tuple(d.shape) == (B, H, W) and d.dtype == torch.float32
        for b in range(B):
            clipped, ratio = float((d[b] == 0).float().mean()), float(d[b].std() / d[b].mean())
            print(f"{B}x{H}x{W} image {b}: clipped {100 * clipped:.1f} %, std / mean {ratio:.3f}")
            assert 0.02 <= clipped <= 0.50 and ratio >= 0.25 and float(d[b].min()) == 0.0
    for name in ("dpt_tiny_w", "dpt_tiny_io"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1024 * 1024


@pytest.mark.parametrize("B,H,W", R.TINY_SIZES)
def test_restatement_matches_the_reference_to_fp32_rounding(golden, B, H, W):
    """The same torch operators in the same order as the reference: rel-L2 <= 1e-6 (tests/test_hed_cpu.py's tolerance for its restatement)."""
    sd, io = golden
    mine = R.forward(sd, R.normalize(T(io[f"pixels.{B}x{H}x{W}"])), HEADS, R.TINY["layers"])
    ref = T(io[f"depth.{B}x{H}x{W}"])
    assert tuple(mine.shape) == tuple(ref.shape)
    assert rel_l2(mine, ref) <= 1e-6


@pytest.mark.parametrize("B,H,W", R.TINY_SIZES)
def test_control_stays_near_the_reference(golden, B, H, W):
    """The bf16-storage control (in the HIP path's order: out_conv before the interpolation) against the stored depth.  The figure is printed: it is
    the yardstick of the GPU tests, not a gate; the bounds here only say the control is the same network and does round."""
    sd, io = golden
    ctl = R.control(sd, R.normalize(T(io[f"pixels.{B}x{H}x{W}"])), HEADS, R.TINY["layers"])
    e = rel_l2(ctl, T(io[f"depth.{B}x{H}x{W}"]))
    print(f"{B}x{H}x{W}: control rel-L2 {e:.3e}")
    assert 1e-4 < e < 5e-2


def test_get_size_equals_the_recorded_pairs(golden):
    from anyedit_amd.depth_anything_v2 import get_size
    rec = golden[1]["get_size"]
    assert [tuple(r[:2]) for r in rec.tolist()] == R.GET_SIZE_PAIRS and len(rec) >= 20
    for w, h, nw, nh in rec.tolist():
        assert get_size(w, h) == (nw, nh), (w, h)
        assert R.get_size(w, h) == (nw, nh), (w, h)
        assert nw % 14 == 0 and nh % 14 == 0 and min(nw, nh) >= 518
    assert get_size(518, 518) == (518, 518) and get_size(1036, 518) == (1036, 518)
    with pytest.raises(ValueError):
        get_size(0, 10)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_load_depth_anything_accepts_the_prefix_and_is_strict(golden, prefix, tmp_path):
    from anyedit_amd.checkpoints import load_depth_anything
    sd, _ = golden
    net = _tiny_model()
    assert set(net.state_dict()) == set(sd)
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in net.state_dict().items())
    assert load_depth_anything(net, {prefix + k: v for k, v in sd.items()}) == (prefix.rstrip(".") or "state_dict")
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    gone = "depth_head.scratch.refinenet4.resConfUnit1.conv2.bias"          # in the checkpoint, read by nothing: still required
    with pytest.raises(RuntimeError, match="refinenet4.resConfUnit1.conv2.bias"):
        load_depth_anything(_tiny_model(), {prefix + k: v for k, v in sd.items() if k != gone})
    extra = dict({prefix + k: v for k, v in sd.items()}, **{prefix + "depth_head.readout_projects.0.0.bias": torch.zeros(64)})
    with pytest.raises(RuntimeError, match="readout_projects"):
        load_depth_anything(_tiny_model(), extra)
    mixed = dict(sd)
    mixed["module.pretrained.cls_token"] = mixed.pop("pretrained.cls_token")            # a prefix on some keys only is not a prefix
    with pytest.raises(RuntimeError, match="cls_token"):
        load_depth_anything(_tiny_model(), mixed)
    if prefix == "":
        path = str(tmp_path / "depth_anything_v2_tiny.pth")
        torch.save(sd, path)
        net2 = _tiny_model()
        assert load_depth_anything(net2, path) == "state_dict"
        assert torch.equal(net2.depth_head.scratch.output_conv2[2].weight, sd["depth_head.scratch.output_conv2.2.weight"])


def test_model_keeps_the_reference_names_and_defaults():
    """The default constructor is the reference's ViT-L model: its state-dict names and shapes, built on the meta device."""
    from anyedit_amd.depth_anything_v2 import DepthAnythingV2
    with torch.device("meta"):
        full = DepthAnythingV2()
    sdm = full.state_dict()
    assert full.encoder == "vitl" and full.intermediate_layer_idx["vitl"] == [4, 11, 17, 23]
    shapes = {"pretrained.pos_embed": (1, 1370, 1024), "pretrained.blocks.23.mlp.fc2.weight": (1024, 4096), "depth_head.projects.1.weight": (512, 1024, 1, 1),
              "depth_head.resize_layers.0.weight": (256, 256, 4, 4), "depth_head.resize_layers.1.bias": (512,), "depth_head.resize_layers.3.weight": (1024, 1024, 3, 3),
              "depth_head.scratch.layer4_rn.weight": (256, 1024, 3, 3), "depth_head.scratch.refinenet4.resConfUnit1.conv1.weight": (256, 256, 3, 3),
              "depth_head.scratch.refinenet2.out_conv.bias": (256,), "depth_head.scratch.output_conv1.weight": (128, 256, 3, 3),
              "depth_head.scratch.output_conv2.0.weight": (32, 128, 3, 3), "depth_head.scratch.output_conv2.2.weight": (1, 32, 1, 1)}
    for k, s in shapes.items():
        assert tuple(sdm[k].shape) == s, k
    assert not any(k.startswith("depth_head.resize_layers.2") or "layer1_rn.bias" in k for k in sdm)
    head = [k for k in sdm if k.startswith("depth_head.")]
    assert len(head) == 8 + 6 + 4 + 4 * 10 + 2 + 4, len(head)


def test_what_is_not_built_is_refused_with_the_reason():
    from anyedit_amd.depth_anything_v2 import DepthAnythingV2, DPTHead
    with pytest.raises(ValueError, match="no ViT-g head has been published"):
        DepthAnythingV2(encoder="vitg")
    with pytest.raises(ValueError, match="batch norm"):
        DepthAnythingV2(encoder="vits", use_bn=True, config=R.TINY_TOWER)
    with pytest.raises(ValueError, match="readout"):
        DepthAnythingV2(encoder="vits", use_clstoken=True, config=R.TINY_TOWER)
    with pytest.raises(ValueError, match="supported"):
        DepthAnythingV2(encoder="vitx")
    with pytest.raises(ValueError, match="four increasing block indices"):
        DepthAnythingV2(config=R.TINY_TOWER, **dict(R.TINY, layers=(0, 1, 2, 4)))
    with pytest.raises(ValueError, match="multiples of 8"):
        DPTHead(64, features=32, out_channels=(12, 32, 64, 64))
    with pytest.raises(ValueError, match="multiple of 16"):
        DPTHead(64, features=24, out_channels=(16, 32, 64, 64))
    net = _tiny_model()
    with pytest.raises(ValueError, match="whole number"):
        net(torch.zeros(1, 3, 20, 28))
    with pytest.raises(ValueError, match="GPU only"):
        net(torch.zeros(1, 3, 28, 28))
    with pytest.raises(TypeError, match="BGR uint8"):
        net.infer_image(np.zeros((20, 20, 3), np.float32))


def test_colour_table_is_matplotlibs_spectral_r():
    from anyedit_amd.depth_anything_v2 import spectral_r_table
    table = spectral_r_table()
    assert table.dtype == np.uint8 and table.shape == (256, 3)
    assert tuple(table[0]) == (94, 79, 162) and len({tuple(r) for r in table.tolist()}) > 200
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps.get_cmap("Spectral_r")
    assert np.array_equal(table, (cmap(np.arange(256))[:, :3] * 255).astype(np.uint8))
    idx = (np.arange(35 * 20) % 256).astype(np.uint8).reshape(35, 20)
    ref = (cmap(idx)[:, :, :3] * 255)[:, :, ::-1].astype(np.uint8)          # visual_condition_tool.py:133, BGR for cv2.imwrite
    assert np.array_equal(table[idx], ref[:, :, ::-1]), "the table indexed by the uint8 map is the reference's colour image with its channels in RGB order"


def test_index_arithmetic_equals_the_recorded_result(golden):
    _, io = golden
    B, H, W = R.TINY_SIZES[0]
    d = io[f"depth.{B}x{H}x{W}"][0]
    idx = R.depth_index(d)
    assert idx.dtype == np.uint8 and np.array_equal(idx, io["index.u8"])
    assert int(idx.min()) == 0 and int(idx.max()) == 255 and len(np.unique(idx)) > 100


def test_img2depth_hands_the_model_bgr_and_writes_rgb(tmp_path):
    """`img2depth` with the model replaced by a recording stand-in: the array it hands over is the file's pixels with the channel axis reversed
    (cv2.imread's order), the file it writes holds the returned RGB colour image unflipped, and a .txt list names the files."""
    from PIL import Image
    from anyedit_amd.tools.tool import img2depth, depth_filenames
    rgb = (R.smooth_pixels(1, 40, 28, seed=5)[0].permute(1, 2, 0).numpy() * 255.0).round().astype(np.uint8)
    assert not np.array_equal(rgb, rgb[:, :, ::-1])
    src, dst, lst = (str(tmp_path / n) for n in ("in.png", "out.png", "list.txt"))
    Image.fromarray(rgb).save(src)
    with open(lst, "w") as f:
        f.write(src + "\n")
    colour = (np.arange(40 * 28 * 3) % 251).astype(np.uint8).reshape(40, 28, 3)
    seen = []

    class StandIn:
        def colour_image(self, raw):
            seen.append(np.array(raw))
            return colour

    assert img2depth(src, dst, StandIn()) == dst
    assert np.array_equal(np.array(Image.open(dst)), colour)
    assert img2depth(lst, dst, StandIn()) == dst and depth_filenames(lst) == [src]
    assert len(seen) == 2 and all(np.array_equal(s, rgb[:, :, ::-1]) for s in seen)


def test_entry_points_are_declared_and_bound():
    from anyedit_amd import _lib
    header = open(os.path.join(ROOT, "include", "anyedit_hip.h")).read()
    for name in ("ae_dpt_reassemble_bf16", "ae_dpt_resize_bf16", "ae_dpt_relu_bf16", "ae_dpt_tail_bf16", "ae_depth_resize_minmax_f32", "ae_depth_colorize_u8"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"
