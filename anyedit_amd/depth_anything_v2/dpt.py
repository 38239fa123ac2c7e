"""Depth Anything V2 on HIP: mirror of AnyEdit_Collection/other_modules/depth_anything_v2/dpt.py and util/blocks.py (the annotator of the
`visual_depth` condition, visual_condition_tool.py:111-134).  Same class names, constructor arguments and state-dict keys (`pretrained.*` = the DINOv2
tower's; `depth_head.projects.N`, `depth_head.resize_layers.{0,1,3}`, `depth_head.scratch.layerN_rn`, `depth_head.scratch.refinenetN.{out_conv,
resConfUnit1, resConfUnit2}`, `depth_head.scratch.output_conv1`, `depth_head.scratch.output_conv2.{0,2}`), so a `depth_anything_v2_vit{s,b,l}.pth`
loads with strict=True.

Launches of one head on a gh x gw grid of patches (activations between launches are bf16 channels-last rows [B*H*W, C]; `# bf16:` marks every stored
activation, tests/dpt_ref.py rounds at exactly those points for its control):
    reassemble   levels 1, 2: ops.gemm (projects, +bias) -> ops.gemm (the ConvTranspose2d of stride k as a [k k oc, oc] product, fp32) ->
                 ops.dpt_reassemble (skip the class rows, + bias, one rounding, scatter to (gh k) x (gw k));
                 levels 3, 4: ops.gemm (projects, fp32) -> ops.dpt_reassemble (k = 1); level 4 then ops.conv3x3(stride=2)
    4 x          ops.conv3x3          layerN_rn (no bias)
    per ResidualConvUnit              relu(x) (ops.dpt_relu, or the second output of the resize that produced x), ops.conv3x3, ops.relu_,
                                      ops.conv3x3(residual=x)
    per FeatureFusionBlock            ops.gemm (out_conv) on the LOW-resolution rows, then ops.dpt_resize to the next level's size with the next
                                      block's resConfUnit1 output as its addend (blocks.py:133) and relu(result) as its second output
    end          ops.conv3x3 (output_conv1), ops.dpt_resize to 14 gh x 14 gw, ops.conv3x3 (output_conv2[0]), ops.dpt_tail (ReLU, 32 -> 1 in fp32, ReLU)
`detect` adds ops.depth_resize_minmax and ops.depth_colorize.

One piece of work is removed: a FeatureFusionBlock ends with `interpolate` followed by the 1x1 `out_conv` (blocks.py:144-146).  Both are linear and
the bilinear weights of a pixel sum to 1 (so the bias passes through), hence out_conv(interpolate(x)) = interpolate(out_conv(x)): the product runs on
the low-resolution map, a quarter of the rows.  In fp32 the two orders differ by rounding only (3.6e-7 at magnitude 2).

Not built: use_bn, use_clstoken, the ViT-g head (none is published), the metric-depth variants.  `refinenet4.resConfUnit1` is in the checkpoint and
nothing reads it (refinenet4 has one input): it is carried for the state dict.
"""
import os
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from anyedit_amd import ops
from anyedit_amd.ldm.modules.encoders.dino_vision import DINOV2_VITB14, DINOV2_VITL14, DINOV2_VITS14, DinoVisionTransformer

BF16 = torch.bfloat16
PATCH = 14
# dpt.py:164-169 intermediate_layer_idx and dinov2.py's geometry per model_name
ENCODERS = {"vits": (DINOV2_VITS14, (2, 5, 8, 11)), "vitb": (DINOV2_VITB14, (2, 5, 8, 11)), "vitl": (DINOV2_VITL14, (4, 11, 17, 23))}
_TABLE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spectral_r.txt")


def spectral_r_table():
    """matplotlib's `Spectral_r` as img2depth uses it (visual_condition_tool.py:126, :133): uint8 [256, 3], row i = (cmap(i)[:3] * 255) truncated, RGB.
    Stored as data beside this module (tools/gen_golden_dpt.py writes it from matplotlib; tests/test_dpt_cpu.py compares where matplotlib imports)."""
    t = np.loadtxt(_TABLE_FILE, dtype=np.int64)
    if t.shape != (256, 3) or t.min() < 0 or t.max() > 255:
        raise ValueError(f"{_TABLE_FILE}: expected 256 rows of three values in 0 .. 255")
    return t.astype(np.uint8)


def get_size(width, height, input_size=518, multiple_of=PATCH):
    """util/transform.py:62-107 Resize.get_size as image2tensor configures it (dpt.py:198-206: keep_aspect_ratio, 'lower_bound', ensure_multiple_of=14):
    both sides scaled by the larger of input_size / width and input_size / height, rounded to the nearest multiple (half to even, np.round), and
    rounded UP instead where that falls below input_size.  Returns (new_width, new_height)."""
    if width < 1 or height < 1:
        raise ValueError(f"get_size: bad image size {width} x {height}")
    scale = max(input_size / width, input_size / height)

    def constrain(x):
        y = int(np.round(x / multiple_of) * multiple_of)
        if y < input_size:
            y = int(np.ceil(x / multiple_of) * multiple_of)
        return y
    return constrain(scale * width), constrain(scale * height)


def _f(t):
    return t.detach().float().contiguous()


class ResidualConvUnit(nn.Module):
    """blocks.py:29-80 without batch norm: out = conv2(relu(conv1(relu(x)))) + x.  Holds the parameters; DPTHead runs the arithmetic."""

    def __init__(self, features, activation=None, bn=False):
        super().__init__()
        if bn:
            raise ValueError("ResidualConvUnit: bn=True is not built (the published Depth Anything V2 heads have no batch norm)")
        self.conv1 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv2 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.parameters()):
            self._pk = types.SimpleNamespace(w1=ops.pack_conv3x3(self.conv1.weight.detach().float()), b1=_f(self.conv1.bias),
                                             w2=ops.pack_conv3x3(self.conv2.weight.detach().float()), b2=_f(self.conv2.bias))
        return self._pk


class FeatureFusionBlock(nn.Module):
    """blocks.py:83-148 as dpt.py:12-21 builds it (no deconv, no batch norm, no expand, align_corners=True)."""

    def __init__(self, features, activation=None, deconv=False, bn=False, expand=False, align_corners=True, size=None):
        super().__init__()
        if deconv or bn or expand or not align_corners:
            raise ValueError("FeatureFusionBlock: only the form the DPT head builds is covered (deconv=False, bn=False, expand=False, align_corners=True)")
        self.out_conv = nn.Conv2d(features, features, kernel_size=1, stride=1, padding=0, bias=True)
        self.resConfUnit1 = ResidualConvUnit(features, activation, bn)
        self.resConfUnit2 = ResidualConvUnit(features, activation, bn)
        self.size = size

    def packed(self):
        if ops.cache_stale(self, "_pk", *self.out_conv.parameters()):
            self._pk = types.SimpleNamespace(w=ops.pack_linear(self.out_conv.weight), b=_f(self.out_conv.bias))
        return self._pk


class DPTHead(nn.Module):
    """dpt.py:38-150.  `run(tokens, B, gh, gw)` takes the four normed token buffers of the tower, [B * (1 + gh gw), C] bf16 with each image's class row
    first, and returns fp32 depth [B, 14 gh, 14 gw] in a buffer that is static per (B, gh, gw)."""

    def __init__(self, in_channels, features=256, use_bn=False, out_channels=(256, 512, 1024, 1024), use_clstoken=False):
        super().__init__()
        if use_bn:
            raise ValueError("DPTHead: use_bn=True is not built (the published Depth Anything V2 checkpoints have no batch norm)")
        if use_clstoken:
            raise ValueError("DPTHead: use_clstoken=True is not built (the published Depth Anything V2 checkpoints have no readout projections)")
        out_channels = tuple(out_channels)
        if len(out_channels) != 4 or any(c < 8 or c % 8 for c in out_channels) or in_channels % 8:
            raise ValueError(f"DPTHead: four level widths and the token width must be multiples of 8 (16 bytes per lane), got {out_channels} on {in_channels}")
        if features < 16 or features % 16:
            raise ValueError(f"DPTHead: features={features} must be a multiple of 16 (output_conv1 halves it; the kernels take 8 channels per lane)")
        self.use_clstoken = False
        self.in_channels, self.features, self.out_channels = in_channels, features, out_channels
        self.projects = nn.ModuleList([nn.Conv2d(in_channels, oc, kernel_size=1, stride=1, padding=0) for oc in out_channels])
        self.resize_layers = nn.ModuleList([
            nn.ConvTranspose2d(out_channels[0], out_channels[0], kernel_size=4, stride=4, padding=0),
            nn.ConvTranspose2d(out_channels[1], out_channels[1], kernel_size=2, stride=2, padding=0),
            nn.Identity(),
            nn.Conv2d(out_channels[3], out_channels[3], kernel_size=3, stride=2, padding=1)])
        s = self.scratch = nn.Module()
        for n, oc in enumerate(out_channels, 1):
            setattr(s, f"layer{n}_rn", nn.Conv2d(oc, features, kernel_size=3, stride=1, padding=1, bias=False))
        s.stem_transpose = None
        for n in (1, 2, 3, 4):
            setattr(s, f"refinenet{n}", FeatureFusionBlock(features))
        s.output_conv1 = nn.Conv2d(features, features // 2, kernel_size=3, stride=1, padding=1)
        s.output_conv2 = nn.Sequential(nn.Conv2d(features // 2, 32, kernel_size=3, stride=1, padding=1), nn.ReLU(True),
                                       nn.Conv2d(32, 1, kernel_size=1, stride=1, padding=0), nn.ReLU(True), nn.Identity())
        self._ws = {}

    def packed(self):
        """bf16 weight images and fp32 biases of everything outside the fusion blocks, rebuilt when a parameter changes.  A ConvTranspose2d weight
        [ci, co, k, k] becomes the [k k co, ci] matrix whose row (ky k + kx) co_n + co holds tap (ky, kx) of output channel co."""
        s = self.scratch
        own = [p for m in (self.projects, self.resize_layers, s.layer1_rn, s.layer2_rn, s.layer3_rn, s.layer4_rn, s.output_conv1, s.output_conv2) for p in m.parameters()]
        if ops.cache_stale(self, "_pk", *own):
            c3 = lambda conv: ops.pack_conv3x3(conv.weight.detach().float())
            tr = []
            for i in (0, 1):
                w = self.resize_layers[i].weight.detach().float()
                k = w.shape[-1]
                tr.append((w.permute(2, 3, 1, 0).reshape(k * k * w.shape[1], w.shape[0]).to(BF16).contiguous(), _f(self.resize_layers[i].bias), k))
            self._pk = types.SimpleNamespace(
                proj=[(ops.pack_linear(p.weight), _f(p.bias)) for p in self.projects], tr=tr, down=(c3(self.resize_layers[3]), _f(self.resize_layers[3].bias)),
                rn=[c3(getattr(s, f"layer{n}_rn")) for n in (1, 2, 3, 4)], oc1=(c3(s.output_conv1), _f(s.output_conv1.bias)),
                oc2=(c3(s.output_conv2[0]), _f(s.output_conv2[0].bias)), wp=_f(s.output_conv2[2].weight).reshape(-1), bp=_f(s.output_conv2[2].bias).reshape(-1))
        return self._pk

    def _workspace(self, B, gh, gw, dev):
        key = (B, gh, gw, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = {}
        return ws

    def _rcu(self, unit, x, xr, B, H, W, buf, tag):
        """ResidualConvUnit on rows x with xr = relu(x): conv1, ReLU in place, conv2 + x."""
        p = unit.packed()
        Fc = self.features
        c1, _, _ = ops.conv3x3(xr, p.w1, p.b1, B, H, W, out=buf(tag + ".c1", (B * H * W, Fc)))                 # bf16: conv1 output
        ops.relu_(c1)
        y, _, _ = ops.conv3x3(c1, p.w2, p.b2, B, H, W, residual=x, out=buf(tag + ".y", (B * H * W, Fc)))       # bf16: conv2 + bias + x, one rounding
        return y

    @torch.no_grad()
    def run(self, tokens, B, gh, gw):
        if len(tokens) != 4:
            raise ValueError(f"DPTHead: expected the token rows of four blocks, got {len(tokens)}")
        if gh < 1 or gw < 1 or PATCH * gh > ops.DPT_MAX_SIDE or PATCH * gw > ops.DPT_MAX_SIDE:
            raise ValueError(f"DPTHead: a {gh} x {gw} grid of patches is refused (images of 14 .. {ops.DPT_MAX_SIDE} pixels a side are covered)")
        dev = tokens[0].device
        M, Fc, oc = B * (1 + gh * gw), self.features, self.out_channels
        for t in tokens:
            if t.dtype != BF16 or tuple(t.shape) != (M, self.in_channels) or not t.is_contiguous():
                raise ValueError(f"DPTHead: token rows must be contiguous bf16 [{M}, {self.in_channels}], got {t.dtype} {tuple(t.shape)}")
        ws = self._workspace(B, gh, gw, dev)

        def buf(name, shape, dtype=BF16):
            b = ws.get(name)
            if b is None:
                b = ws[name] = torch.empty(*shape, dtype=dtype, device=dev)
            return b

        pk = self.packed()
        sizes = [(4 * gh, 4 * gw), (2 * gh, 2 * gw), (gh, gw), ((gh - 1) // 2 + 1, (gw - 1) // 2 + 1)]
        levels = []
        for i in (0, 1):                                                                                        # dpt.py:129-130, ConvTranspose2d levels
            wt, bt, k = pk.tr[i]
            p = ops.gemm(tokens[i], pk.proj[i][0], pk.proj[i][1], out=buf(f"proj{i}", (M, oc[i])))              # bf16: projects[i] output, all token rows
            prod = ops.gemm(p, wt, None, out_f32=True, out=buf(f"prod{i}", (M, k * k * oc[i]), torch.float32))  # fp32: the transposed convolution's product
            levels.append(ops.dpt_reassemble(prod, bt, B, gh, gw, k, out=buf(f"level{i}", (B * sizes[i][0] * sizes[i][1], oc[i]))))  # bf16: level map
        for i in (2, 3):                                                                                        # Identity, and the input of the stride-2 convolution
            prod = ops.gemm(tokens[i], pk.proj[i][0], None, out_f32=True, out=buf(f"prod{i}", (M, oc[i]), torch.float32))         # fp32: projects[i] product
            levels.append(ops.dpt_reassemble(prod, pk.proj[i][1], B, gh, gw, 1, out=buf(f"level{i}", (B * gh * gw, oc[i]))))       # bf16: projects[i] output
        h4, w4 = sizes[3]
        levels[3], _, _ = ops.conv3x3(levels[3], pk.down[0], pk.down[1], B, gh, gw, stride=2, out=buf("down", (B * h4 * w4, oc[3])))  # bf16: level-4 map
        rn = []
        for i in range(4):
            H, W = sizes[i]
            rn.append(ops.conv3x3(levels[i], pk.rn[i], None, B, H, W, out=buf(f"rn{i}", (B * H * W, Fc)))[0])   # bf16: layerN_rn output
        s = self.scratch
        # refinenet4 has one input: resConfUnit2 on layer_4_rn
        H, W = sizes[3]
        x = rn[3]
        xr = ops.dpt_relu(x, out=buf("f3.xr", (B * H * W, Fc)))
        for i in (3, 2, 1, 0):
            blk = getattr(s, f"refinenet{i + 1}")
            y = self._rcu(blk.resConfUnit2, x, xr, B, H, W, buf, f"f{i}.u2")
            o = ops.gemm(y, blk.packed().w, blk.packed().b, out=buf(f"f{i}.o", (B * H * W, Fc)))               # bf16: out_conv on the low-resolution rows
            if i == 0:
                break
            Hn, Wn = sizes[i - 1]
            nxt = getattr(s, f"refinenet{i}")
            sr = ops.dpt_relu(rn[i - 1], out=buf(f"f{i - 1}.sr", (B * Hn * Wn, Fc)))
            res = self._rcu(nxt.resConfUnit1, rn[i - 1], sr, B, Hn, Wn, buf, f"f{i - 1}.u1")
            x, xr = ops.dpt_resize(o, B, H, W, Hn, Wn, addend=res, out=buf(f"f{i - 1}.x", (B * Hn * Wn, Fc)),   # bf16: interpolate + skip_add, one rounding
                                   relu_out=buf(f"f{i - 1}.xr", (B * Hn * Wn, Fc)))
            H, W = Hn, Wn
        H2, W2 = 2 * H, 2 * W                                                                                    # refinenet1: scale_factor=2
        path1 = ops.dpt_resize(o, B, H, W, H2, W2, out=buf("path1", (B * H2 * W2, Fc)))                          # bf16: path_1
        c, _, _ = ops.conv3x3(path1, pk.oc1[0], pk.oc1[1], B, H2, W2, out=buf("oc1", (B * H2 * W2, Fc // 2)))   # bf16: output_conv1
        Hf, Wf = PATCH * gh, PATCH * gw
        up = ops.dpt_resize(c, B, H2, W2, Hf, Wf, out=buf("up", (B * Hf * Wf, Fc // 2)))                         # bf16: dpt.py:147
        y, _, _ = ops.conv3x3(up, pk.oc2[0], pk.oc2[1], B, Hf, Wf, out=buf("oc2", (B * Hf * Wf, 32)))            # bf16: output_conv2[0] before its ReLU
        return ops.dpt_tail(y, pk.wp, pk.bp, B, Hf, Wf, out=buf("depth", (B, Hf, Wf), torch.float32))

    def forward(self, out_features, patch_h, patch_w):
        """dpt.py:117-150 on `get_intermediate_layers(..., return_class_token=True)` pairs is not how this head is fed: it reads the tower's token rows
        (class row included) directly.  Use `DepthAnythingV2.forward`, or `run` with the four normed token buffers."""
        raise NotImplementedError("DPTHead.forward: call DPTHead.run(tokens, B, gh, gw) with the tower's normed token rows (DepthAnythingV2.forward does)")


class DepthAnythingV2(nn.Module):
    """dpt.py:153-221.  The reference's constructor arguments, plus two keywords for test geometries: `config` (overrides of the encoder's tower
    geometry, DinoVisionTransformer's argument) and `layers` (the four block indices whose outputs feed the head).

    forward(x)                  fp32 [B, 3, H, W] normalised pixels on the GPU, H and W multiples of 14 -> fp32 depth [B, H, W]
    detect(image, size=None)    fp32 [B, 3, H, W] RGB in [0, 1] (ImageNet normalisation inside the patch launch) -> uint8 colour image [B, h, w, 3]
                                (RGB, `Spectral_r`) at `size` = (h, w), default (H, W): the device part of img2depth
    infer_image(raw_image, input_size=518)   BGR uint8 array [h, w, 3] -> fp32 numpy depth [h, w], as the reference
    colour_image(raw_image, input_size=518)  BGR uint8 array -> RGB uint8 colour image [h, w, 3]
    After the first call of a shape `forward` and `detect` allocate no buffer of their own and never synchronise with the host, run on the current
    stream and may be captured in a graph; what they return are views of buffers that are static per shape: the next call of that shape overwrites them.

    The input resize of `infer_image` is torch's F.interpolate(mode="bicubic", align_corners=False) on the GPU in fp32, where the reference calls
    cv2.resize(INTER_CUBIC) on float64 pixels: the two share the kernel constant a = -0.75 and the half-pixel grid; that equivalence is the
    definition here and is not checked against cv2."""

    def __init__(self, encoder="vitl", features=256, out_channels=(256, 512, 1024, 1024), use_bn=False, use_clstoken=False, config=None, layers=None):
        super().__init__()
        if encoder == "vitg":
            raise ValueError("DepthAnythingV2: encoder='vitg' is refused: no ViT-g head has been published, so there is nothing to load or to test against")
        if encoder not in ENCODERS:
            raise ValueError(f"DepthAnythingV2: encoder {encoder!r} (supported: {sorted(ENCODERS)})")
        if use_bn:
            raise ValueError("DepthAnythingV2: use_bn=True is not built (the published checkpoints have no batch norm)")
        if use_clstoken:
            raise ValueError("DepthAnythingV2: use_clstoken=True is not built (the published checkpoints have no readout projections)")
        base, idx = ENCODERS[encoder]
        cfg = dict(base)
        cfg.update(config or {})
        if cfg["patch_size"] != PATCH:
            raise ValueError(f"DepthAnythingV2: patch_size {cfg['patch_size']}: the head is written for {PATCH}-pixel patches (dpt.py:147, :177)")
        idx = tuple(int(i) for i in (layers if layers is not None else idx))
        if len(idx) != 4 or list(idx) != sorted(set(idx)) or idx[0] < 0 or idx[-1] >= cfg["depth"]:
            raise ValueError(f"DepthAnythingV2: layers must be four increasing block indices in [0, {cfg['depth']}), got {idx}")
        self.intermediate_layer_idx = {encoder: list(idx)}
        self.encoder = encoder
        self.pretrained = DinoVisionTransformer(cfg)
        self.depth_head = DPTHead(self.pretrained.embed_dim, features, use_bn, out_channels=out_channels, use_clstoken=use_clstoken)
        self._out = {}

    def _depth(self, x, normalize):
        tw = self.pretrained
        idx = self.intermediate_layer_idx[self.encoder]
        ws = tw.run(x, n_blocks=idx[-1] + 1, normalize=normalize)
        px = x[0] if isinstance(x, (list, tuple)) else x
        B, gh, gw = ws.ones.shape[0], px.shape[2] // PATCH, px.shape[3] // PATCH
        return self.depth_head.run([tw._normed(ws, i + 1) for i in idx], B, gh, gw)      # get_intermediate_layers(norm=True): the class row stays in the buffer

    @torch.no_grad()
    def forward(self, x):
        """dpt.py:176-184."""
        return self._depth(x, normalize=False)

    def _table(self, dev):
        t = self.__dict__.get("_lut")
        if t is None or t.device != dev:
            t = self.__dict__["_lut"] = torch.from_numpy(spectral_r_table()).to(dev)
        return t

    @torch.no_grad()
    def detect(self, image, size=None, want_depth=False):
        depth = self._depth(image, normalize=True)
        B, H, W = depth.shape
        h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
        key = (B, H, W, h, w, str(depth.device))
        o = self._out.get(key)
        if o is None:
            e = lambda *s, dt: torch.empty(*s, dtype=dt, device=depth.device)
            o = self._out[key] = types.SimpleNamespace(depth=e(B, h, w, dt=torch.float32), mm=e(B, 2, dt=torch.float32), rgb=e(B, h, w, 3, dt=torch.uint8))
        table = self._table(depth.device)
        ops.depth_resize_minmax(depth, h, w, out=o.depth, minmax=o.mm)                   # dpt.py:192 and visual_condition_tool.py:131's min / max
        ops.depth_colorize(o.depth, o.mm, table, out=o.rgb)                              # visual_condition_tool.py:131-133
        return (o.rgb, o.depth, o.mm) if want_depth else o.rgb

    def image2tensor(self, raw_image, input_size=518):
        """dpt.py:196-221 up to the normalisation (which `detect` fuses into the patch launch): BGR uint8 [h, w, 3] -> (fp32 [1, 3, H, W] RGB in [0, 1]
        on the model's device, (h, w))."""
        raw = np.asarray(raw_image)
        if raw.ndim != 3 or raw.shape[2] != 3 or raw.dtype != np.uint8:
            raise TypeError(f"DepthAnythingV2: expected a BGR uint8 [h, w, 3] array, got {raw.dtype} {raw.shape}")
        h, w = raw.shape[:2]
        W2, H2 = get_size(w, h, input_size)
        if max(H2, W2) > ops.DPT_MAX_SIDE:
            raise ValueError(f"DepthAnythingV2: a {h} x {w} image would run at {H2} x {W2}; sides up to {ops.DPT_MAX_SIDE} are covered")
        dev = self.pretrained.device
        rgb = torch.from_numpy(np.ascontiguousarray(raw[:, :, ::-1])).to(dev).permute(2, 0, 1).unsqueeze(0).float() / 255.0
        return F.interpolate(rgb, size=(H2, W2), mode="bicubic", align_corners=False).contiguous(), (h, w)

    @torch.no_grad()
    def infer_image(self, raw_image, input_size=518):
        """dpt.py:186-194."""
        image, (h, w) = self.image2tensor(raw_image, input_size)
        _, depth, _ = self.detect(image, size=(h, w), want_depth=True)
        return depth[0].cpu().numpy()

    @torch.no_grad()
    def colour_image(self, raw_image, input_size=518):
        image, (h, w) = self.image2tensor(raw_image, input_size)
        return self.detect(image, size=(h, w))[0].cpu().numpy()
