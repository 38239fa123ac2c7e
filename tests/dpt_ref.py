"""Plain-torch restatement of Depth Anything V2 (AnyEdit_Collection/other_modules/depth_anything_v2/dpt.py, util/blocks.py) over a state dict, for
the tests and tools: `forward` (fp32, the reference's own operator order: in a FeatureFusionBlock the interpolation comes BEFORE the 1x1 out_conv),
`control` (the bf16-storage control of the project's tolerance rule, in the HIP path's order: out_conv on the low-resolution map, then the
interpolation), the detector's arithmetic after the network (`resize_depth`, `depth_index`), and the seeded weights and images the fixtures and the
wider test are built from.  The tower is tests/dino_ref.py's.

`forward` is pinned to the reference's own outputs (tests/golden/dpt_tiny_io.npz, written by tools/gen_golden_dpt.py) by tests/test_dpt_cpu.py.

The control is fp32 arithmetic with every matrix / convolution weight rounded to bf16 as the module packs it and every activation rounded to bf16
exactly where anyedit_amd/depth_anything_v2/dpt.py stores one (its `# bf16:` marks; keep the two in step).  NOT rounded: biases, the ConvTranspose2d
product and the projects product of levels 3 and 4 (fp32 on the HIP path until the bias is added), the 32 -> 1 projection and the depth.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dino_ref

TINY_TOWER = dict(embed_dim=64, num_heads=1, depth=4, patch_size=14, img_size=70, mlp_ratio=4.0, ffn_layer="mlp")
TINY = dict(encoder="vits", features=32, out_channels=(16, 32, 64, 64), layers=(0, 1, 2, 3))
TINY_SIZES = [(2, 70, 70), (1, 42, 56), (2, 14, 14), (1, 28, 98)]          # (B, H, W)
TINY_SEED = 7           # of 40 seeds tried, one of nine at which every stored image meets the fixture condition (tools/gen_golden_dpt.py)
WIDE_TOWER = dict(embed_dim=384, num_heads=6, depth=12, patch_size=14, img_size=518, mlp_ratio=4.0, ffn_layer="mlp")
WIDE = dict(encoder="vits", features=64, out_channels=(48, 96, 192, 384), layers=(2, 5, 8, 11))
GET_SIZE_PAIRS = [(640, 480), (480, 640), (518, 518), (1036, 518), (518, 1036), (100, 100), (37, 200), (200, 37), (1920, 1080), (1080, 1920), (500, 375),
                  (375, 500), (1024, 768), (14, 14), (519, 517), (777, 1234), (1500, 511), (259, 259), (1000, 1000), (3000, 2000), (333, 518), (525, 700)]
DEPTH_MEAN = 1.0        # the pre-ReLU depth of the first image after `rescale_tail`: mean = standard deviation = 1


def _round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def split(sd):
    """`pretrained.*` and `depth_head.*` of a DepthAnythingV2 state dict, prefixes stripped"""
    return ({k[len("pretrained."):]: v for k, v in sd.items() if k.startswith("pretrained.")},
            {k[len("depth_head."):]: v for k, v in sd.items() if k.startswith("depth_head.")})


def _interp(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)


def _head(hd, feats, gh, gw, ctl, want_pre=False):
    """DPTHead.forward (dpt.py:117-150) on the four patch-token tensors [B, G, C]; ctl: the bf16-storage control in the HIP path's order."""
    st = _round if ctl else (lambda t: t)
    f = lambda k: hd[k].float()
    w = (lambda k: _round(hd[k].float())) if ctl else f
    B = feats[0].shape[0]
    out = []
    for i, x in enumerate(feats):
        x = st(x.float()).permute(0, 2, 1).reshape(B, -1, gh, gw)
        q = f"projects.{i}."
        r = f"resize_layers.{i}."
        if i < 2:
            x = st(F.conv2d(x, w(q + "weight"), f(q + "bias")))                                          # bf16: projects[i] output
            k = hd[r + "weight"].shape[-1]
            x = st(F.conv_transpose2d(x, w(r + "weight"), None, stride=k) + f(r + "bias").view(1, -1, 1, 1))   # bf16: level map (fp32 product + bias, one rounding)
        else:
            x = st(F.conv2d(x, w(q + "weight"), None) + f(q + "bias").view(1, -1, 1, 1))                 # bf16: projects[i] output (fp32 product + bias)
            if i == 3:
                x = st(F.conv2d(x, w(r + "weight"), f(r + "bias"), stride=2, padding=1))                 # bf16: level-4 map
        out.append(x)
    rn = [st(F.conv2d(x, w(f"scratch.layer{n + 1}_rn.weight"), None, padding=1)) for n, x in enumerate(out)]     # bf16: layerN_rn output

    def rcu(q, x):
        c = st(F.conv2d(F.relu(x), w(q + "conv1.weight"), f(q + "conv1.bias"), padding=1))               # bf16: conv1 output
        return st(F.conv2d(F.relu(c), w(q + "conv2.weight"), f(q + "conv2.bias"), padding=1) + x)        # bf16: conv2 + bias + x, one rounding

    def fusion(n, x, skip, size):                                                                        # blocks.py:129-146, the reference's order
        q = f"scratch.refinenet{n}."
        if skip is not None:
            x = x + rcu(q + "resConfUnit1.", skip)
        x = rcu(q + "resConfUnit2.", x)
        x = _interp(x, size)
        return F.conv2d(x, f(q + "out_conv.weight"), f(q + "out_conv.bias"))

    sizes = [t.shape[2:] for t in rn]
    if not ctl:
        p = fusion(4, rn[3], None, sizes[2])
        p = fusion(3, p, rn[2], sizes[1])
        p = fusion(2, p, rn[1], sizes[0])
        p = fusion(1, p, rn[0], (2 * sizes[0][0], 2 * sizes[0][1]))
    else:                                                                                                # the HIP order: out_conv on the low-resolution map
        x = rn[3]
        for n in (4, 3, 2, 1):
            q = f"scratch.refinenet{n}."
            y = rcu(q + "resConfUnit2.", x)
            o = st(F.conv2d(y, w(q + "out_conv.weight"), f(q + "out_conv.bias")))                        # bf16: out_conv on the low-resolution rows
            if n == 1:
                break
            res = rcu(f"scratch.refinenet{n - 1}.resConfUnit1.", rn[n - 2])
            x = st(_interp(o, sizes[n - 2]) + res)                                                       # bf16: interpolate + skip_add, one rounding
        p = st(_interp(o, (2 * sizes[0][0], 2 * sizes[0][1])))                                           # bf16: path_1
    c = st(F.conv2d(p, w("scratch.output_conv1.weight"), f("scratch.output_conv1.bias"), padding=1))     # bf16: output_conv1
    c = st(_interp(c, (14 * gh, 14 * gw)))                                                               # bf16: dpt.py:147
    y = st(F.conv2d(c, w("scratch.output_conv2.0.weight"), f("scratch.output_conv2.0.bias"), padding=1)) # bf16: output_conv2[0] before its ReLU
    pre = F.conv2d(F.relu(y), f("scratch.output_conv2.2.weight"), f("scratch.output_conv2.2.bias"))      # fp32: the 32 -> 1 projection
    return pre[:, 0] if want_pre else F.relu(F.relu(pre))[:, 0]                                          # output_conv2[3] and forward's F.relu (:182)


@torch.no_grad()
def _model(sd, x, heads, layers, ctl, want_pre=False):
    tower, head = split(sd)
    gh, gw = x.shape[-2] // 14, x.shape[-1] // 14
    r = dino_ref.dino_forward(tower, x, heads, bf16_storage=ctl, n_blocks=max(layers) + 1)
    feats = [r["normed"][i + 1][:, 1:] for i in layers]                                                  # get_intermediate_layers(norm=True), patch tokens
    return _head(head, feats, gh, gw, ctl, want_pre)


def forward(sd, x, heads, layers, want_pre=False):
    """DepthAnythingV2.forward (dpt.py:176-184) in fp32: x [B, 3, H, W] normalised pixels -> depth [B, H, W]; want_pre: the map before the last
    two ReLUs."""
    return _model(sd, x, heads, layers, False, want_pre)


def control(sd, x, heads, layers):
    return _model(sd, x, heads, layers, True)


def resize_depth(depth, h, w):
    """infer_image's resize (dpt.py:192): [B, H, W] -> [B, h, w]"""
    return _interp(depth[:, None], (h, w))[:, 0]


def depth_index(depth):
    """visual_condition_tool.py:131-132 on one fp32 numpy map: the uint8 index into the colour map"""
    depth = np.asarray(depth, dtype=np.float32)
    depth = (depth - depth.min()) / (depth.max() - depth.min()) * 255.0
    return depth.astype(np.uint8)


def get_size(width, height, input_size=518, multiple_of=14):
    """util/transform.py:62-107 with image2tensor's arguments, written as the reference writes it (numpy scalars)."""
    def constrain(x, min_val):
        y = (np.round(x / multiple_of) * multiple_of).astype(int)
        if y < min_val:
            y = (np.ceil(x / multiple_of) * multiple_of).astype(int)
        return y
    scale_height, scale_width = input_size / height, input_size / width
    if scale_width > scale_height:
        scale_height = scale_width
    else:
        scale_width = scale_height
    return int(constrain(np.float64(scale_width * width), input_size)), int(constrain(np.float64(scale_height * height), input_size))


# ------------------------------------------------------------------------------------------------ seeded weights and images
def seeded_head(C, features, out_channels, seed=0):
    """Seeded `depth_head.*` weights: fan-in scaled matrices (activations keep their scale through the head), biases N(0, 0.3) so that a dropped
    bias shows.  Every weight that feeds a bf16 GEMM or convolution is a bf16 value; biases and the 32 -> 1 projection are full fp32."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std: _round(torch.randn(*s, generator=g) * std)
    b = lambda c: torch.randn(c, generator=g) * 0.3
    hd = {}
    for i, oc in enumerate(out_channels):
        hd[f"projects.{i}.weight"], hd[f"projects.{i}.bias"] = n(oc, C, 1, 1, std=C ** -0.5), b(oc)
    for i, k in ((0, 4), (1, 2)):
        oc = out_channels[i]
        hd[f"resize_layers.{i}.weight"], hd[f"resize_layers.{i}.bias"] = n(oc, oc, k, k, std=oc ** -0.5), b(oc)
    oc = out_channels[3]
    hd["resize_layers.3.weight"], hd["resize_layers.3.bias"] = n(oc, oc, 3, 3, std=(9 * oc) ** -0.5), b(oc)
    for i, oc in enumerate(out_channels, 1):
        hd[f"scratch.layer{i}_rn.weight"] = n(features, oc, 3, 3, std=(9 * oc) ** -0.5)
    for i in (1, 2, 3, 4):
        q = f"scratch.refinenet{i}."
        hd[q + "out_conv.weight"], hd[q + "out_conv.bias"] = n(features, features, 1, 1, std=features ** -0.5), b(features)
        for u in ("resConfUnit1.", "resConfUnit2."):
            for c in ("conv1.", "conv2."):
                hd[q + u + c + "weight"], hd[q + u + c + "bias"] = n(features, features, 3, 3, std=math.sqrt(2.0 / (9 * features))), b(features)
    hd["scratch.output_conv1.weight"], hd["scratch.output_conv1.bias"] = n(features // 2, features, 3, 3, std=(9 * features) ** -0.5), b(features // 2)
    hd["scratch.output_conv2.0.weight"], hd["scratch.output_conv2.0.bias"] = n(32, features // 2, 3, 3, std=math.sqrt(2.0 / (9 * (features // 2)))), b(32)
    hd["scratch.output_conv2.2.weight"] = torch.randn(1, 32, 1, 1, generator=g) / math.sqrt(32.0)
    hd["scratch.output_conv2.2.bias"] = torch.randn(1, generator=g) * 0.3
    return hd


def seeded_state_dict(tower_cfg, features, out_channels, seed=0):
    cfg = dict(in_chans=3, init_values=1.0)
    cfg.update(tower_cfg)
    sd = {"pretrained." + k: v for k, v in dino_ref.seeded_state_dict(cfg, seed=seed).items()}
    sd.update({"depth_head." + k: v for k, v in seeded_head(cfg["embed_dim"], features, out_channels, seed=seed + 1).items()})
    return sd


def rescale_tail(sd, pre):
    """Rescales the last 1x1 layer in place so that `pre`, the map it gave before the final ReLU, gets mean = standard deviation = DEPTH_MEAN: about
    16 % of the depth is then clipped to 0 and the rest spreads over a range of its own size.  (With the initial weights the depth is a near-constant
    map, and every comparison on it would be vacuous.)  Returns (gain, shift)."""
    mu, s = float(pre.double().mean()), float(pre.double().std())
    a = DEPTH_MEAN / s
    c = DEPTH_MEAN - a * mu
    wk, bk = "depth_head.scratch.output_conv2.2.weight", "depth_head.scratch.output_conv2.2.bias"
    sd[wk] = (sd[wk].double() * a).float()
    sd[bk] = (sd[bk].double() * a + c).float()
    return a, c


def smooth_pixels(B, H, W, seed):
    """fp32 [B, 3, H, W] RGB in [0, 1]: low-frequency waves per channel, a disc and a bar per image (values are multiples of 1 / 255)."""
    out = np.zeros((B, 3, H, W), np.float32)
    for i in range(B):
        rng = np.random.RandomState(seed * 31 + i)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64) / H, np.arange(W, dtype=np.float64) / W, indexing="ij")
        img = np.zeros((H, W, 3))
        for c in range(3):
            v = 128.0
            for _ in range(4):
                fy, fx, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * np.pi)
                v = v + 28.0 * np.sin(2 * np.pi * (fy * yy + fx * xx) + ph)
            img[..., c] = v
        cy, cx, rad = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.15, 0.3)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2] += 45.0 * np.sign(rng.randn(3))
        x0 = rng.uniform(0.1, 0.6)
        img[:, (xx[0] > x0) & (xx[0] < x0 + 0.15)] -= 35.0
        out[i] = (np.clip(np.round(img), 0, 255) / 255.0).astype(np.float32).transpose(2, 0, 1)
    return torch.from_numpy(out)


def normalize(px):
    return dino_ref.normalize(px)
