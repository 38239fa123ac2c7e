"""Plain-torch restatement of the HED edge detector (AnyEdit_Collection/other_modules/HED/__init__.py) for the tests and tools: the network
(`forward`, fp32 or fp64), the detector's arithmetic after it (`mean_logits`, `edge_value`, `edge_map`), the bf16-storage control (`control`), and
the seeded weights and smooth images the fixtures and the full-width tests are built from.

The network is pinned to the reference's own outputs (tests/golden/hed_tiny_io.npz, written by tools/gen_golden_hed.py) by tests/test_hed_cpu.py.
The detector's arithmetic is NOT checked against cv2, which is not installed where the fixtures are made: `cv2.resize(e, (W, H), INTER_LINEAR)`
when enlarging is restated as `F.interpolate(size=(H, W), mode="bilinear", align_corners=False)` — both are documented as bilinear interpolation
with half-pixel centres, source coordinate (dst + 0.5) * src / dst - 0.5, clamped at the edges — followed by the reference's own lines: mean over
the five maps, sigmoid in float64, * 255, clip, astype(uint8) (truncation), 255 - v (cv2.bitwise_not).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (64, 128, 256, 512, 512)
LAYERS = (2, 2, 3, 3, 3)
TINY = dict(channels=(16, 32, 64, 64, 64), layers=(2, 2, 3, 3, 3))
TINY_SIZES = [(50, 38), (64, 48), (33, 47)]
NORM = (124.0, 116.0, 104.0)
LOGIT_STD = 2.5


def layers_of(sd):
    """convolutions per block, read off the state dict's keys"""
    return tuple(1 + max(int(k.split(".")[2]) for k in sd if k.startswith(f"block{n}.convs.")) for n in range(1, 6))


def _net(sd, x, dtype, conv_weight, store):
    p = {k: v.to(dtype) for k, v in sd.items()}
    h = x.to(dtype) - p["norm"].view(1, 3, 1, 1)
    outs = []
    for n, layers in enumerate(layers_of(sd), 1):
        if n > 1:
            h = F.max_pool2d(h, kernel_size=(2, 2), stride=(2, 2))
        for m in range(layers):
            h = store(F.relu(F.conv2d(h, conv_weight(n, m, p[f"block{n}.convs.{m}.weight"]), p[f"block{n}.convs.{m}.bias"], padding=1)))
        outs.append(F.conv2d(h, p[f"block{n}.projection.weight"], p[f"block{n}.projection.bias"]))
    return outs


@torch.no_grad()
def forward(sd, x, dtype=torch.float32):
    """ControlNetHED_Apache2.__call__ (:44-51): x [B, 3, H, W] -> the five projections [B, 1, h, w] in `dtype`."""
    return _net(sd, x, dtype, lambda n, m, w: w, lambda h: h)


@torch.no_grad()
def control(sd, x):
    """The same network with the storage precision of the HIP path and nothing else of it: fp32 weights in the first convolution, bf16 weights in
    the other twelve, every activation rounded to bf16 after its convolution + ReLU, fp32 accumulation, fp32 projections."""
    r = lambda t: t.bfloat16().float()
    return _net(sd, x, torch.float32, lambda n, m, w: w if (n, m) == (1, 0) else r(w), r)


def resize(side, H, W):
    return F.interpolate(side, size=(H, W), mode="bilinear", align_corners=False)


def mean_logits(sides, H, W):
    """:68-70 up to the sigmoid: [B, H, W] in the dtype of `sides` ([B, 1, h, w] or [B, h, w])."""
    sides = [s if s.dim() == 4 else s.unsqueeze(1) for s in sides]
    return torch.stack([resize(s, H, W)[:, 0] for s in sides], 0).mean(0)


def edge_value(logits):
    """:70-71 before the truncation: 255 * sigmoid in float64, clipped to [0, 255]"""
    return (255.0 / (1.0 + torch.exp(-logits.double()))).clamp(0.0, 255.0)


def edge_map(sides, H, W, invert=True):
    """:68-73 on fp32 side maps: uint8 [B, H, W]"""
    v = edge_value(mean_logits([s.float() for s in sides], H, W)).to(torch.uint8)
    return 255 - v if invert else v


# ------------------------------------------------------------------------------------------------ seeded weights and images
def seeded_state_dict(channels=CHANNELS, layers=LAYERS, seed=0):
    """He-scaled weights (activations keep their scale through the depth), biases of the activations' order of magnitude so that a dropped bias
    shows, an integer-valued `norm`.  The twelve wide convolutions' weights are bf16 values (the fixtures store their bit patterns); the first
    convolution and the projections are full fp32."""
    g = torch.Generator().manual_seed(seed)
    sd = {"norm": torch.tensor(NORM).view(1, 3, 1, 1)}
    cin = 3
    for n, (c, l) in enumerate(zip(channels, layers), 1):
        for m in range(l):
            w = torch.randn(c, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
            sd[f"block{n}.convs.{m}.weight"] = w if (n, m) == (1, 0) else w.bfloat16().float()
            sd[f"block{n}.convs.{m}.bias"] = torch.randn(c, generator=g) * 10.0
            cin = c
        sd[f"block{n}.projection.weight"] = torch.randn(1, c, 1, 1, generator=g) / math.sqrt(c)
        sd[f"block{n}.projection.bias"] = torch.randn(1, generator=g)
    return sd


def rescale_heads(sd, sides, H, W):
    """Rescales the five projection heads in place so that, for the image that gave `sides`, every resized side map has zero mean and their mean
    map has standard deviation LOGIT_STD: without it the logits reach +-300 and the edge map is all 0 or 255.  The resize is linear and keeps
    constants, so an affine change of a head is the same affine change of its resized map.  Returns the scale and shift applied per head."""
    maps = [resize(s.double(), H, W) for s in sides]
    stats = [(float(m.mean()), float(m.std())) for m in maps]
    total = torch.stack([(m - mu) / sd_ for m, (mu, sd_) in zip(maps, stats)], 0).mean(0)
    gain = LOGIT_STD / float(total.std())
    applied = []
    for n, (mu, sd_) in enumerate(stats, 1):
        a = gain / sd_
        w, b = sd[f"block{n}.projection.weight"], sd[f"block{n}.projection.bias"]
        sd[f"block{n}.projection.weight"] = (w.double() * a).float()
        sd[f"block{n}.projection.bias"] = ((b.double() - mu) * a).float()
        applied.append((a, mu))
    return applied


def smooth_image(H, W, seed):
    """A smooth uint8 [H, W, 3] image with a few edges: low-frequency waves per channel, a disc and a bar."""
    rng = np.random.RandomState(seed)
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
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def to_nchw(image_u8):
    """uint8 [H, W, 3] (numpy) -> fp32 [1, 3, H, W], as HEDdetector.__call__ :64-65"""
    return torch.from_numpy(np.ascontiguousarray(image_u8)).float().permute(2, 0, 1).unsqueeze(0).contiguous()


def smooth_logits(B, h, w, seed, std=LOGIT_STD):
    """A smooth fp32 [B, h, w] map of the given standard deviation (per batch): white noise blurred, for the fuse kernel's tests."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 1, h + 8, w + 8, generator=g, dtype=torch.float64)
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64)
    k2 = (k[:, None] * k[None, :] / 256.0).view(1, 1, 5, 5)
    z = F.conv2d(F.conv2d(z, k2), k2)
    z = z - z.mean()
    return (z * (std / float(z.std())))[:, 0].float().contiguous()


def smooth_sides(B, H, W, seed):
    """Five fp32 side maps [B, 1, H >> k, W >> k] as a network might give them: one shared smooth field of standard deviation LOGIT_STD plus a
    weaker field per level, averaged down to the level's size."""
    base = smooth_logits(B, H, W, seed)
    return [F.adaptive_avg_pool2d((base + smooth_logits(B, H, W, seed * 7 + k + 1, std=0.8)).unsqueeze(1), (H >> k, W >> k)).contiguous() for k in range(5)]
