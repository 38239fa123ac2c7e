"""Plain-torch restatement of the UniFormer backbone (AnyEdit_Collection/other_modules/uniformer/mmseg/models/backbones/uniformer.py, eval mode,
windows=False, hybrid=False) over a state dict, for the tests and tools: `forward` (fp32 or fp64, the reference's own operator order: BatchNorm, then
the 1x1 convolution), `control` (the bf16-storage control of the project's tolerance rule), the BatchNorm fold (`fold_bn`), and the seeded weights
and smooth images the fixtures and the wider test are built from.

`forward` is pinned to the reference's own outputs (tests/golden/uniformer_tiny_io.npz, written by tools/gen_golden_uniformer.py) by
tests/test_uniformer_cpu.py.

The control is fp32 arithmetic with every matrix rounded to bf16 as anyedit_amd/uniformer packs it (conv1 and mlp.fc1 of a CBlock AFTER their
BatchNorm has been folded in, in fp32) and every activation rounded to bf16 exactly where the module stores one (its `# bf16:` marks; keep the two in
step), the input pixels and the LayerNorm outputs that feed a matrix product included.  NOT rounded: the depthwise weights, biases, LayerNorm
parameters, the attention probabilities, and the four fp32 output maps.
"""
import math

import torch
import torch.nn.functional as F

S_GEOMETRY = dict(layers=(3, 4, 8, 3), embed_dim=(64, 128, 320, 512), head_dim=64)
TINY = dict(layers=(1, 1, 2, 1), embed_dim=(16, 32, 64, 64), head_dim=32)
TINY_SIZES = [(2, 64, 48), (1, 72, 56), (1, 40, 104)]          # (B, H, W); 72x56: maps 18x14, 9x7, 4x3, 2x1, both floors
TINY_SEED = 0           # the first seed tried; every stored level meets the fixture condition (tools/gen_golden_uniformer.py prints the figures)
WIDE = dict(layers=(1, 1, 2, 1), embed_dim=(64, 128, 320, 512), head_dim=64)
FIXTURE_BAND = (1e-4, 5e-2)    # the control's rel-L2 against the reference, every stored level
BN_EPS, PATCH_LN_EPS, BLOCK_LN_EPS = 1e-5, 1e-5, 1e-6


def _round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def layers_of(sd):
    return tuple(1 + max(int(k.split(".")[1]) for k in sd if k.startswith(f"blocks{n}.")) for n in range(1, 5))


def fold_bn(weight, bias, gamma, beta, mean, var, eps=BN_EPS):
    """BatchNorm (eval) in front of a 1x1 convolution as one affine map: ([N, K] weight, [N] bias) in the dtype of the arguments."""
    w = weight.reshape(weight.shape[0], -1)
    s = gamma / torch.sqrt(var + eps)
    return w * s[None, :], bias + w @ (beta - mean * s)


def _ln(x, w, b, eps):
    """LayerNorm over the channels of an NCHW map"""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def _net(sd, x, head_dim, ctl, dtype):
    st = _round if ctl else (lambda t: t)
    p = lambda k: sd[k].to(dtype)
    wr = (lambda k: _round(p(k))) if ctl else p
    c1 = lambda t, w, b: F.conv2d(t, w.reshape(w.shape[0], -1, 1, 1), b)

    def bn_conv(t, bn, conv):
        args = (p(conv + "weight"), p(conv + "bias"), p(bn + "weight"), p(bn + "bias"), p(bn + "running_mean"), p(bn + "running_var"))
        if ctl:
            w, b = fold_bn(*args)
            return c1(t, _round(w), b)
        t = F.batch_norm(t, args[4], args[5], args[2], args[3], False, 0.0, BN_EPS)
        return c1(t, args[0], args[1])

    def cblock(q, t):
        C = t.shape[1]
        t = st(t + F.conv2d(t, p(q + "pos_embed.weight"), p(q + "pos_embed.bias"), padding=1, groups=C))
        u = st(bn_conv(t, q + "norm1.", q + "conv1."))
        u = st(F.conv2d(u, p(q + "attn.weight"), p(q + "attn.bias"), padding=2, groups=C))
        t = st(t + c1(u, wr(q + "conv2.weight"), p(q + "conv2.bias")))
        u = st(F.gelu(bn_conv(t, q + "norm2.", q + "mlp.fc1.")))
        return st(t + c1(u, wr(q + "mlp.fc2.weight"), p(q + "mlp.fc2.bias")))

    def sablock(q, t):
        B, C, H, W = t.shape
        heads = C // head_dim
        t = st(t + F.conv2d(t, p(q + "pos_embed.weight"), p(q + "pos_embed.bias"), padding=1, groups=C))
        t = t.flatten(2).transpose(1, 2)
        y = st(F.layer_norm(t, (C,), p(q + "norm1.weight"), p(q + "norm1.bias"), BLOCK_LN_EPS))
        qkv = st(F.linear(y, wr(q + "attn.qkv.weight"), p(q + "attn.qkv.bias"))).reshape(B, H * W, 3, heads, head_dim).permute(2, 0, 3, 1, 4)
        a = ((qkv[0] @ qkv[1].transpose(-2, -1)) * head_dim ** -0.5).softmax(-1)
        o = st((a @ qkv[2]).transpose(1, 2).reshape(B, H * W, C))
        t = st(t + F.linear(o, wr(q + "attn.proj.weight"), p(q + "attn.proj.bias")))
        y = st(F.layer_norm(t, (C,), p(q + "norm2.weight"), p(q + "norm2.bias"), BLOCK_LN_EPS))
        u = st(F.gelu(F.linear(y, wr(q + "mlp.fc1.weight"), p(q + "mlp.fc1.bias"))))
        t = st(t + F.linear(u, wr(q + "mlp.fc2.weight"), p(q + "mlp.fc2.bias")))
        return t.transpose(1, 2).reshape(B, C, H, W)

    h = st(x.to(dtype))
    outs = []
    for n, depth in enumerate(layers_of(sd), 1):
        q = f"patch_embed{n}."
        k = sd[q + "proj.weight"].shape[-1]
        h = st(F.conv2d(h, wr(q + "proj.weight"), p(q + "proj.bias"), stride=k))
        h = st(_ln(h, p(q + "norm.weight"), p(q + "norm.bias"), PATCH_LN_EPS))
        for i in range(depth):
            h = (cblock if n <= 2 else sablock)(f"blocks{n}.{i}.", h)
        outs.append(_ln(h, p(f"norm{n}.weight"), p(f"norm{n}.bias"), BLOCK_LN_EPS).contiguous())
    return tuple(outs)


@torch.no_grad()
def forward(sd, x, head_dim, dtype=torch.float32):
    """UniFormer.forward (:383-422): x [B, 3, H, W] -> the four NCHW maps in `dtype`."""
    return _net(sd, x, head_dim, False, dtype)


@torch.no_grad()
def control(sd, x, head_dim):
    return _net(sd, x, head_dim, True, torch.float32)


# ------------------------------------------------------------------------------------------------ seeded weights and images
def seeded_state_dict(layers, embed_dim, head_dim, mlp_ratio=4, in_chans=3, seed=0):
    """A full backbone state dict, the BatchNorm buffers (num_batches_tracked too) included.  Matrices from N(0, 1 / fan_in) (the second one of
    every residual branch at half of that, so the rows keep their scale through the depth), biases from N(0, 0.1^2); the depthwise kernels from
    N(0, 1 / k^2); LayerNorm and BatchNorm weights from U(0.5, 1.5), their biases from N(0, 0.2^2); BatchNorm running means from N(0, 0.5^2) and
    running variances spread over [0.5, 2] (log-uniform): a fold that drops the mean, the variance, gamma or beta moves the outputs by far more than
    any bound.  The matrices the module rounds to bf16 as they are (everything but a CBlock's conv1 and mlp.fc1, which are folded first) hold bf16
    values."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bfv = lambda t: t.bfloat16().float()
    sd = {}

    def affine(q, C):
        sd[q + "weight"], sd[q + "bias"] = 0.5 + torch.rand(C, generator=g), 0.2 * rn(C)

    def bnorm(q, C):
        affine(q, C)
        sd[q + "running_mean"] = 0.5 * rn(C)
        sd[q + "running_var"] = 0.5 * torch.exp(torch.rand(C, generator=g) * math.log(4.0))
        sd[q + "num_batches_tracked"] = torch.tensor(100, dtype=torch.long)

    def dw(q, C, k):
        sd[q + "weight"], sd[q + "bias"] = rn(C, 1, k, k) / k, 0.1 * rn(C)

    def mat(q, shape, gain=1.0, exact=True):
        fan_in = int(torch.tensor(shape[1:]).prod())
        w = rn(*shape) * gain / math.sqrt(fan_in)
        sd[q + "weight"], sd[q + "bias"] = (bfv(w) if exact else w), 0.1 * rn(shape[0])

    cin = in_chans
    for n, (C, depth) in enumerate(zip(embed_dim, layers), 1):
        k = 4 if n == 1 else 2
        mat(f"patch_embed{n}.proj.", (C, cin, k, k))
        affine(f"patch_embed{n}.norm.", C)
        hid = int(C * mlp_ratio)
        for i in range(depth):
            q = f"blocks{n}.{i}."
            dw(q + "pos_embed.", C, 3)
            if n <= 2:
                bnorm(q + "norm1.", C)
                mat(q + "conv1.", (C, C, 1, 1), exact=False)
                mat(q + "conv2.", (C, C, 1, 1), gain=0.5)
                dw(q + "attn.", C, 5)
                bnorm(q + "norm2.", C)
                mat(q + "mlp.fc1.", (hid, C, 1, 1), exact=False)
                mat(q + "mlp.fc2.", (C, hid, 1, 1), gain=0.5)
            else:
                affine(q + "norm1.", C)
                mat(q + "attn.qkv.", (3 * C, C), gain=1.5)
                mat(q + "attn.proj.", (C, C), gain=0.5)
                affine(q + "norm2.", C)
                mat(q + "mlp.fc1.", (hid, C))
                mat(q + "mlp.fc2.", (C, hid), gain=0.5)
        affine(f"norm{n}.", C)
        cin = C
    return sd


BF16_KEYS = ("proj.weight", "conv2.weight", "qkv.weight", "fc2.weight")


def stored_as_bf16(key, sd):
    """True for the matrices `seeded_state_dict` draws as bf16 values (the fixtures store their bit patterns)"""
    if key.endswith("mlp.fc1.weight"):
        return sd[key].dim() == 2                   # Mlp's Linear; CMlp's convolution is folded with norm2 first
    return key.endswith(BF16_KEYS)


def smooth_pixels(B, H, W, seed):
    """Smooth fp32 [B, 3, H, W] images as a normalised photograph might be (values of order 1), every image of the batch drawn differently: low-frequency
    waves per channel, a disc and a bar."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: float(lo + (hi - lo) * torch.rand(1, generator=g))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64) / H, torch.arange(W, dtype=torch.float64) / W, indexing="ij")
    img = torch.zeros(B, 3, H, W, dtype=torch.float64)
    for b in range(B):
        for c in range(3):
            v = torch.full((H, W), u(-0.3, 0.3), dtype=torch.float64)
            for _ in range(4):
                v = v + 0.45 * torch.sin(2 * math.pi * (u(0.5, 3.0) * yy + u(0.5, 3.0) * xx) + u(0.0, 2 * math.pi))
            img[b, c] = v
        cy, cx, rad = u(0.3, 0.7), u(0.3, 0.7), u(0.15, 0.3)
        disc = ((yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2).to(torch.float64)
        img[b] += 0.8 * disc * torch.sign(torch.randn(3, 1, 1, generator=g, dtype=torch.float64))
        x0 = u(0.1, 0.6)
        img[b] -= 0.6 * ((xx > x0) & (xx < x0 + 0.15)).to(torch.float64)
    return img.float().contiguous()
