"""Plain-torch restatement of the UPerNet head and the end of EncoderDecoder.simple_test (AnyEdit_Collection/other_modules/uniformer/mmseg/models/
decode_heads/uper_head.py, psp_head.py, decode_head.py, segmentors/encoder_decoder.py; eval mode, align_corners=False) over the head's state dict,
for the tests and tools: `head_forward` (fp32 or fp64, the reference's own operator order: convolution, BatchNorm, ReLU), `head_control` (the
bf16-storage control of the project's tolerance rule), the two resizes and the argmax (`resize_twice`, `segment`), the BatchNorm fold, the bin and tap
arithmetic of the kernels in exact integers, `rescale_size`, and the seeded weights the fixtures and the wider test are built from.

`head_forward` and `segment` are pinned to the reference's own outputs (tests/golden/upernet_tiny_io.npz, written by tools/gen_golden_upernet.py) by
tests/test_upernet_cpu.py.

The control is fp32 arithmetic with every matrix rounded to bf16 as anyedit_amd/uniformer/upernet.py packs it (AFTER its BatchNorm has been folded
in, in fp32) and every activation rounded to bf16 exactly where the module stores one (its `# bf16:` marks; keep the two in step): the four input
maps, the pooled rows, every ConvModule output, every resized map, every top-down sum.  NOT rounded: the folded biases, conv_seg's bias, the fp32
logits and everything behind them.
"""
import math

import torch
import torch.nn.functional as F

TINY_HEAD = dict(in_channels=(16, 32, 64, 64), channels=32, num_classes=150, pool_scales=(1, 2, 3, 6))
WIDE_HEAD = dict(in_channels=(64, 128, 320, 512), channels=512, num_classes=150, pool_scales=(1, 2, 3, 6))
TINY_SEED = 0            # the first seed tried that meets the fixture conditions (tools/gen_golden_upernet.py prints the figures)
SECOND_ORI = {"2x64x48": (45, 67), "1x72x56": (101, 83), "1x40x104": (23, 57)}      # a second ori_shape per image that the input does not divide
BN_EPS = 1e-5
MIN_DISTINCT, NEAR_SHARE = 8, 0.40     # fixture conditions: distinct labels per image; share of pixels with a top-two margin below 3 e_ctl


def _round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def fold_bn_after_conv(weight, gamma, beta, mean, var, eps=BN_EPS):
    """BatchNorm (eval) behind a bias-free convolution as one convolution: (weight scaled per output channel, bias) in the dtype of the arguments"""
    s = gamma / torch.sqrt(var + eps)
    return weight * s.view(-1, 1, 1, 1), beta - mean * s


def resize(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)


def _head(sd, maps, pool_scales, ctl, dtype):
    st = _round if ctl else (lambda t: t)
    p = lambda k: sd[k].to(dtype)

    def conv_module(q, t):
        """ConvModule BEFORE its ReLU"""
        w = p(q + "conv.weight")
        bn = [p(q + "bn." + n) for n in ("weight", "bias", "running_mean", "running_var")]
        pad = w.shape[-1] // 2
        if ctl:
            wf, bf = fold_bn_after_conv(w, *bn)
            return F.conv2d(t, _round(wf), bf, padding=pad)
        return F.batch_norm(F.conv2d(t, w, None, padding=pad), bn[2], bn[3], bn[0], bn[1], False, 0.0, BN_EPS)

    maps = [st(m.to(dtype)) for m in maps]
    x = maps[3]
    outs = [x]
    for k, s in enumerate(pool_scales):
        t = st(F.adaptive_avg_pool2d(x, s))
        t = st(F.relu(conv_module(f"psp_modules.{k}.1.", t)))
        outs.append(st(resize(t, x.shape[2:])))
    psp = F.relu(st(conv_module("bottleneck.", torch.cat(outs, 1))))                  # stored before the ReLU; the readers apply it
    lat = [st(F.relu(conv_module(f"lateral_convs.{i}.", maps[i]))) for i in range(3)] + [psp]
    for i in range(3, 0, -1):
        lat[i - 1] = st(lat[i - 1] + resize(lat[i], lat[i - 1].shape[2:]))
    fpn = [F.relu(st(conv_module(f"fpn_convs.{i}.", lat[i]))) for i in range(3)] + [psp]
    size0 = fpn[0].shape[2:]
    cat = torch.cat([fpn[0]] + [st(resize(f, size0)) for f in fpn[1:]], 1)
    y = F.relu(st(conv_module("fpn_bottleneck.", cat)))
    w = p("conv_seg.weight")
    return F.conv2d(y, _round(w) if ctl else w, p("conv_seg.bias"))


@torch.no_grad()
def head_forward(sd, maps, pool_scales=(1, 2, 3, 6), dtype=torch.float32):
    """UPerHead.forward: the four NCHW maps -> logits [B, num_classes, h0, w0] in `dtype`"""
    return _head(sd, maps, pool_scales, False, dtype)


@torch.no_grad()
def head_control(sd, maps, pool_scales=(1, 2, 3, 6)):
    return _head(sd, maps, pool_scales, True, torch.float32)


def resize_twice(logits, mid, out):
    """encode_decode's resize to the network input's size, then whole_inference's to ori_shape (always applied there, the identity at equal sizes)"""
    return resize(resize(logits, mid), out)


def segment(logits, mid, out, softmax=True):
    """simple_test: labels int64 [B, Ho, Wo]"""
    full = resize_twice(logits, mid, out)
    return (full.softmax(1) if softmax else full).argmax(1)


def top_two_margin(full):
    top = full.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


# ------------------------------------------------------------------------------------------------ the kernels' integer arithmetic
def pool_bins(n, s):
    """[(start, end)] of AdaptiveAvgPool's s bins along an axis of length n: floor(i n / s) .. ceil((i + 1) n / s)"""
    return [((i * n) // s, -((-(i + 1) * n) // s)) for i in range(s)]


def pool_rows64(x, scales):
    """x float64 [B, H, W, C] -> the rows of ops.ppm_pool in float64, [B, sum s s, C]"""
    B, H, W, C = x.shape
    rows = []
    for s in scales:
        for y0, y1 in pool_bins(H, s):
            for x0, x1 in pool_bins(W, s):
                rows.append(x[:, y0:y1, x0:x1].reshape(B, -1, C).mean(1))
    return torch.stack(rows, 1)


def axis_taps(n, N):
    """align_corners=False along one axis in exact integers: (i0, i1 int64 [N], l1 float64 [N]); source coordinate ((2 d + 1) n - N) / (2 N) clamped
    at 0, upper neighbour clamped at n - 1"""
    d = torch.arange(N, dtype=torch.int64)
    num = torch.clamp((2 * d + 1) * n - N, min=0)
    i0 = num // (2 * N)
    return i0, torch.clamp(i0 + 1, max=n - 1), (num - i0 * 2 * N).to(torch.float64) / (2 * N)


def bilinear64(x, H, W):
    """x float64 [B, h, w, C] -> (the exact align_corners=False resize [B, H, W, C], the four taps' magnitudes summed)"""
    h, w = x.shape[1:3]
    y0, y1, ly = axis_taps(h, H)
    x0, x1, lx = axis_taps(w, W)
    ly, lx = ly.view(1, H, 1, 1), lx.view(1, 1, W, 1)
    a00, a01, a10, a11 = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return (1 - ly) * ((1 - lx) * a00 + lx * a01) + ly * ((1 - lx) * a10 + lx * a11), a00.abs() + a01.abs() + a10.abs() + a11.abs()


def rescale_size(old_size, scale):
    """mmcv's rescale_size for a (long edge, short edge) scale: (w, h) -> (new w, new h)"""
    w, h = old_size
    f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(f) + 0.5), int(h * float(f) + 0.5)


# ------------------------------------------------------------------------------------------------ seeded weights
def stored_as_bf16(key):
    """the matrices `seeded_head_state_dict` draws as bf16 values (the fixtures store their bit patterns)"""
    return key.endswith("conv.weight") or key == "conv_seg.weight"


def seeded_head_state_dict(in_channels, channels, num_classes, pool_scales, seed=0):
    """The head's full state dict (num_batches_tracked included).  Convolutions He-scaled, N(0, 2 / fan_in), drawn as bf16 values; every BatchNorm
    with gamma from U(0.5, 1.5), beta from N(0.1, 0.2^2), running means from N(0, 0.5^2) and running variances spread over [0.5, 2] (log-uniform): a
    fold that drops any one of the four moves the logits by far more than any bound; conv_seg from N(0, 0.5^2) (bf16 values), its bias N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bfv = lambda t: t.bfloat16().float()
    sd = {}

    def conv_module(q, cin, cout, k):
        sd[q + "conv.weight"] = bfv(rn(cout, cin, k, k) * math.sqrt(2.0 / (cin * k * k)))
        sd[q + "bn.weight"] = 0.5 + torch.rand(cout, generator=g)
        sd[q + "bn.bias"] = 0.1 + 0.2 * rn(cout)
        sd[q + "bn.running_mean"] = 0.5 * rn(cout)
        sd[q + "bn.running_var"] = 0.5 * torch.exp(torch.rand(cout, generator=g) * math.log(4.0))
        sd[q + "bn.num_batches_tracked"] = torch.tensor(100, dtype=torch.long)

    sd["conv_seg.weight"] = bfv(0.5 * rn(num_classes, channels, 1, 1))
    sd["conv_seg.bias"] = 0.1 * rn(num_classes)
    for k in range(len(pool_scales)):
        conv_module(f"psp_modules.{k}.1.", in_channels[-1], channels, 1)
    conv_module("bottleneck.", in_channels[-1] + len(pool_scales) * channels, channels, 3)
    for i, c in enumerate(in_channels[:-1]):
        conv_module(f"lateral_convs.{i}.", c, channels, 1)
        conv_module(f"fpn_convs.{i}.", channels, channels, 3)
    conv_module("fpn_bottleneck.", len(in_channels) * channels, channels, 3)
    return sd
