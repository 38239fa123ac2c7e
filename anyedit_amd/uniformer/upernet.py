"""UPerNet head and the segmentor around it on HIP: mirror of AnyEdit_Collection/other_modules/uniformer/mmseg/models/decode_heads/uper_head.py
(with psp_head.py's PPM, decode_head.py's BaseDecodeHead and mmcv's ConvModule) and segmentors/encoder_decoder.py, as seg_config.py and
configs/_base_/models/upernet_uniformer.py assemble them for `img2seg`, the annotator of the `visual_segment` condition.  Same class names,
constructor keywords and state-dict keys (`decode_head.psp_modules.0.1.conv.weight`, `decode_head.lateral_convs.1.bn.running_var`,
`decode_head.conv_seg.bias`, ...), so an mmseg checkpoint loads strictly (checkpoints.load_segmentor).  Inference only: eval mode, BatchNorm on its
running statistics folded into the convolution in fp32 (ops.fold_bn_after_conv), dropout an identity, every resize `align_corners=False`.

Launches of one `UPerHead.forward_rows` on the backbone's four bf16 row maps (17, whatever the sizes), then one for the segment map:
    ops.ppm_pool                       the four AdaptiveAvgPool2d of the pyramid                                             [B * 50, C3]
    ops.gemm, EPI_RELU                 the four 1x1 ConvModules at once: their weights stacked, each scale keeps its own columns
    ops.resize_concat, 5 sources       cat([x, resize(ppm_k)...])                                                            [.., C3 + 4 ch]
    ops.conv3x3                        bottleneck, BEFORE its ReLU (both readers are resize_concat launches: the read flag)
    ops.gemm, EPI_RELU (3 x)           lateral_convs
    ops.resize_concat + addend (3 x)   laterals[i - 1] += resize(laterals[i]), in place, from the top
    ops.conv3x3 (3 x)                  fpn_convs, BEFORE their ReLU (read flag)
    ops.resize_concat, 4 sources       cat([fpn_0, resize(fpn_1), resize(fpn_2), resize(psp)])                               [.., 4 ch]
    ops.conv3x3, ops.relu_             fpn_bottleneck
    ops.gemm, fp32 output              conv_seg (weight rows padded with zeros to a multiple of 4)                           [.., 152] fp32
    ops.seg_argmax                     both resizes of simple_test, the argmax and palette[label]; the softmax is left out (strictly increasing)
Activations between launches are bf16 channels-last rows; the maps never go through NCHW.  No host synchronisation: capturable in a graph.

Not built (each refused with a message): `test_cfg.mode='slide'`, flips, `aug_test`, training mode, `align_corners=True`, more than 256 classes, the
auxiliary head (it never runs at inference; its checkpoint entries are skipped), a neck."""
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from anyedit_amd import ops

IMG_MEAN, IMG_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)     # configs/_base_/datasets/ade20k.py img_norm_cfg, after BGR -> RGB
IMG_SCALE = (2048, 512)                                                    # test_pipeline's MultiScaleFlipAug img_scale, keep_ratio=True
MAX_CLASSES = ops.SEG_MAX_CLASSES


def _f32(t):
    return t.detach().float().contiguous()


def _only_bn_relu(conv_cfg, norm_cfg, act_cfg):
    if conv_cfg is not None:
        raise NotImplementedError(f"ConvModule: conv_cfg={conv_cfg} is not built (plain Conv2d only)")
    if not norm_cfg or norm_cfg.get("type") not in ("BN", "SyncBN"):
        raise NotImplementedError(f"ConvModule: norm_cfg={norm_cfg} is not built (BatchNorm folded into the convolution only)")
    if not act_cfg or act_cfg.get("type") != "ReLU":
        raise NotImplementedError(f"ConvModule: act_cfg={act_cfg} is not built (ReLU only)")


class ConvModule(nn.Module):
    """mmcv.cnn.ConvModule as the head uses it: Conv2d(bias=False) -> BatchNorm2d -> ReLU, kernel 1 or 3 (padding k // 2).  `packed()` is the
    convolution with the BatchNorm folded in: a bf16 weight image and an fp32 bias."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None, norm_cfg=dict(type="BN"), act_cfg=dict(type="ReLU"),
                 inplace=True):
        super().__init__()
        _only_bn_relu(conv_cfg, norm_cfg, act_cfg)
        if kernel_size not in (1, 3) or padding != kernel_size // 2:
            raise NotImplementedError(f"ConvModule: kernel {kernel_size} with padding {padding} is not built (1x1, and 3x3 with padding 1)")
        if in_channels % 8 or out_channels % 8:
            raise ValueError(f"ConvModule: {in_channels} -> {out_channels} channels: both must be multiples of 8 (16 bytes per lane)")
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)
        self.activate = nn.ReLU(inplace=inplace)

    def folded(self):
        """(weight [Cout, Cin, k, k], bias [Cout]) in fp32: the convolution with its BatchNorm folded in"""
        bn = self.bn
        return ops.fold_bn_after_conv(self.conv.weight.detach().float(), bn.weight.detach().float(), bn.bias.detach().float(),
                                      bn.running_mean.detach().float(), bn.running_var.detach().float(), bn.eps)

    def packed(self):
        bn = self.bn
        if ops.cache_stale(self, "_pk", self.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var):
            w, b = self.folded()
            self._pk = (ops.pack_linear(w) if self.conv.kernel_size[0] == 1 else ops.pack_conv3x3(w), b.contiguous())
        return self._pk


class PPM(nn.ModuleList):
    """psp_head.py PPM: per pool scale `nn.Sequential(nn.AdaptiveAvgPool2d(s), ConvModule(in_channels, channels, 1))`"""

    def __init__(self, pool_scales, in_channels, channels, conv_cfg, norm_cfg, act_cfg, align_corners):
        super().__init__()
        if align_corners:
            raise NotImplementedError("PPM: align_corners=True is not built (the resize kernels take half-pixel centres)")
        pool_scales = tuple(pool_scales)
        if not 1 <= len(pool_scales) <= ops.PPM_MAX_SCALES or any(s < 1 or s > ops.PPM_MAX_SCALE for s in pool_scales):
            raise NotImplementedError(f"PPM: pool_scales={pool_scales}: 1 .. {ops.PPM_MAX_SCALES} scales of 1 .. {ops.PPM_MAX_SCALE} are built")
        self.pool_scales, self.align_corners, self.in_channels, self.channels = pool_scales, align_corners, in_channels, channels
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        for s in pool_scales:
            self.append(nn.Sequential(nn.AdaptiveAvgPool2d(s), ConvModule(in_channels, channels, 1, conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)))

    def packed(self):
        """the scales' folded 1x1 weights stacked: bf16 [len(scales) * channels, in_channels] and the fp32 bias beside it"""
        tensors = [t for seq in self for t in (seq[1].conv.weight, seq[1].bn.weight, seq[1].bn.bias, seq[1].bn.running_mean, seq[1].bn.running_var)]
        if ops.cache_stale(self, "_pk", *tensors):
            parts = [seq[1].packed() for seq in self]
            self._pk = (torch.cat([w for w, _ in parts]).contiguous(), torch.cat([b for _, b in parts]).contiguous())
        return self._pk


class UPerHead(nn.Module):
    """uper_head.py UPerHead over decode_head.py BaseDecodeHead, with the reference's keywords.  `forward_rows(levels, B)`: the backbone's
    [(rows bf16 [B*h*w, C], h, w)] * 4 -> (logits fp32 rows [B*h0*w0, ld >= num_classes], h0, w0); `forward(levels, B)`: the logits as fp32
    [B, num_classes, h0, w0] (a copy, for comparisons)."""

    def __init__(self, pool_scales=(1, 2, 3, 6), in_channels=None, channels=None, *, num_classes, dropout_ratio=0.1, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type="ReLU"), in_index=(0, 1, 2, 3), input_transform="multiple_select", loss_decode=None, ignore_index=255, sampler=None,
                 align_corners=False):
        super().__init__()
        if align_corners:
            raise NotImplementedError("UPerHead: align_corners=True is not built (the resize kernels take half-pixel centres)")
        if num_classes > MAX_CLASSES or num_classes < 1:
            raise NotImplementedError(f"UPerHead: num_classes={num_classes}: at most {MAX_CLASSES} classes are built (the label image is uint8)")
        if input_transform != "multiple_select" or in_channels is None or len(in_channels) != 4 or tuple(in_index) != (0, 1, 2, 3):
            raise NotImplementedError("UPerHead: four input levels taken in order (input_transform='multiple_select', in_index=[0, 1, 2, 3])")
        if sampler is not None:
            raise NotImplementedError("UPerHead: a pixel sampler belongs to training, which is not built")
        _only_bn_relu(conv_cfg, norm_cfg, act_cfg)
        self.in_channels, self.channels, self.num_classes, self.dropout_ratio = list(in_channels), channels, num_classes, dropout_ratio
        self.conv_cfg, self.norm_cfg, self.act_cfg, self.in_index, self.input_transform = conv_cfg, norm_cfg, act_cfg, list(in_index), input_transform
        self.ignore_index, self.align_corners = ignore_index, align_corners
        kw = dict(conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)
        self.conv_seg = nn.Conv2d(channels, num_classes, kernel_size=1)
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio > 0 else None
        self.psp_modules = PPM(pool_scales, in_channels[-1], channels, align_corners=align_corners, **kw)
        self.bottleneck = ConvModule(in_channels[-1] + len(pool_scales) * channels, channels, 3, padding=1, **kw)
        self.lateral_convs = nn.ModuleList(ConvModule(c, channels, 1, inplace=False, **kw) for c in in_channels[:-1])
        self.fpn_convs = nn.ModuleList(ConvModule(channels, channels, 3, padding=1, inplace=False, **kw) for _ in in_channels[:-1])
        self.fpn_bottleneck = ConvModule(len(in_channels) * channels, channels, 3, padding=1, **kw)
        self.eval()

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("UPerHead: training mode is not built (BatchNorm is folded on its running statistics, dropout is an identity)")
        return super().train(False)

    def _seg(self):
        """conv_seg as an fp32-output product: the weight's rows padded with zeros to a multiple of 4, the bias likewise"""
        m = self.conv_seg
        if ops.cache_stale(self, "_segpk", m.weight, m.bias):
            n = (self.num_classes + 3) // 4 * 4
            w = torch.zeros(n, self.channels, dtype=ops.BF16, device=m.weight.device)
            w[:self.num_classes] = ops.pack_linear(m.weight)
            b = torch.zeros(n, dtype=torch.float32, device=m.weight.device)
            b[:self.num_classes] = m.bias.detach().float()
            self._segpk = (w, b)
        return self._segpk

    @torch.no_grad()
    def forward_rows(self, levels, B):
        if len(levels) != 4:
            raise ValueError(f"UPerHead: expected the backbone's four levels, got {len(levels)}")
        for (r, h, w), c in zip(levels, self.in_channels):
            if r.dtype != ops.BF16 or tuple(r.shape) != (B * h * w, c):
                raise ValueError(f"UPerHead: a level must be bf16 rows [B*h*w, {c}] = [{B * h * w}, {c}], got {r.dtype} {tuple(r.shape)}")
        ch, scales = self.channels, self.psp_modules.pool_scales
        x3, h3, w3 = levels[3]
        c3 = self.in_channels[3]
        # ---- psp_forward
        bins = sum(s * s for s in scales)
        pooled = ops.ppm_pool(x3, B, h3, w3, scales)                                              # bf16 [B * bins, c3]
        pw, pb = self.psp_modules.packed()
        ppm = ops.gemm(pooled, pw, pb, epilogue=ops.EPI_RELU).view(B, bins, len(scales) * ch)      # bf16: relu(bn(conv(pool_k))) in columns k ch ..
        cat = torch.empty(B * h3 * w3, c3 + len(scales) * ch, dtype=ops.BF16, device=x3.device)
        srcs, off = [(x3, h3, w3, 0, False)], 0
        for k, s in enumerate(scales):
            srcs.append((ppm[:, off:off + s * s, k * ch:(k + 1) * ch], s, s, c3 + k * ch, False))
            off += s * s
        ops.resize_concat(srcs, cat, B, h3, w3)                                                    # bf16: cat([x, resize(ppm_k) ...])
        psp, _, _ = ops.conv3x3(cat, *self.bottleneck.packed(), B, h3, w3)                         # bf16: bottleneck BEFORE its ReLU
        # ---- laterals and the top-down sums
        lat = [ops.gemm(levels[i][0], *self.lateral_convs[i].packed(), epilogue=ops.EPI_RELU) for i in range(3)]      # bf16
        sizes = [(h, w) for _, h, w in levels]
        ops.resize_concat([(psp, h3, w3, 0, True)], lat[2], B, *sizes[2], addend=lat[2])          # bf16: lat2 += resize(relu(psp))
        ops.resize_concat([(lat[2], *sizes[2], 0, False)], lat[1], B, *sizes[1], addend=lat[1])   # bf16
        ops.resize_concat([(lat[1], *sizes[1], 0, False)], lat[0], B, *sizes[0], addend=lat[0])   # bf16
        # ---- fpn_convs BEFORE their ReLU, the concat at level 0's size
        fpn = [ops.conv3x3(lat[i], *self.fpn_convs[i].packed(), B, *sizes[i])[0] for i in range(3)]                    # bf16
        h0, w0 = sizes[0]
        cat0 = torch.empty(B * h0 * w0, 4 * ch, dtype=ops.BF16, device=x3.device)
        ops.resize_concat([(fpn[0], h0, w0, 0, True), (fpn[1], *sizes[1], ch, True), (fpn[2], *sizes[2], 2 * ch, True), (psp, h3, w3, 3 * ch, True)],
                          cat0, B, h0, w0)                                                         # bf16: cat of relu(.) resized
        y, _, _ = ops.conv3x3(cat0, *self.fpn_bottleneck.packed(), B, h0, w0)
        ops.relu_(y)                                                                               # bf16: fpn_bottleneck
        return ops.gemm(y, *self._seg(), out_f32=True), h0, w0                                     # fp32: cls_seg (dropout: identity)

    def forward(self, levels, B):
        rows, h, w = self.forward_rows(levels, B)
        return rows[:, :self.num_classes].reshape(B, h, w, self.num_classes).permute(0, 3, 1, 2).contiguous()


def rescale_size(old_size, scale):
    """mmcv/image/geometric.py rescale_size with a (long edge, short edge) scale: (w, h) -> (new w, new h), int(side * factor + 0.5)"""
    w, h = old_size
    long_edge, short_edge = max(scale), min(scale)
    f = min(long_edge / max(h, w), short_edge / min(h, w))
    return int(w * float(f) + 0.5), int(h * float(f) + 0.5)


class EncoderDecoder(nn.Module):
    """encoder_decoder.py EncoderDecoder: `backbone` a `uniformer.UniFormer`, `decode_head` a `UPerHead` (instances, or dicts of their keywords with
    the config's `type` entry).  `test_cfg.mode` must be 'whole'.  CLASSES / PALETTE come from a checkpoint's `meta` (checkpoints.load_segmentor) or
    the `palette=` / `classes=` arguments, which override it."""

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None, pretrained=None, palette=None, classes=None):
        super().__init__()
        from anyedit_amd.uniformer import UniFormer
        if neck is not None:
            raise NotImplementedError("EncoderDecoder: a neck is not built")
        mode = (test_cfg or {}).get("mode", "whole") if isinstance(test_cfg, dict) else getattr(test_cfg, "mode", "whole")
        if mode != "whole":
            raise NotImplementedError(f"EncoderDecoder: test_cfg.mode='{mode}' is not built (whole-image inference only; 'slide' tiles the image)")
        strip = lambda cfg: {k: v for k, v in cfg.items() if k != "type"}
        self.backbone = UniFormer(**strip(backbone)) if isinstance(backbone, dict) else backbone
        self.decode_head = UPerHead(**strip(decode_head)) if isinstance(decode_head, dict) else decode_head
        self.align_corners, self.num_classes = self.decode_head.align_corners, self.decode_head.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self._palette_override, self._classes_override = palette is not None, classes is not None
        self.CLASSES, self.PALETTE = classes, None
        if palette is not None:
            self.set_palette(palette)
        self.eval()
        if isinstance(pretrained, str):
            from anyedit_amd.checkpoints import load_segmentor
            load_segmentor(self, pretrained)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("EncoderDecoder: training mode is not built")
        return super().train(False)

    def set_palette(self, palette):
        pal = np.asarray(palette)
        if pal.shape != (self.num_classes, 3) or pal.min() < 0 or pal.max() > 255:
            raise ValueError(f"EncoderDecoder: the palette must hold {self.num_classes} rows of 3 values 0 .. 255, got shape {pal.shape}")
        self.PALETTE = pal.astype(np.uint8)
        self.__dict__.pop("_pal_dev", None)

    def _palette_on(self, device):
        if self.PALETTE is None:
            raise ValueError("EncoderDecoder: no palette: load a checkpoint whose meta holds PALETTE, or pass palette=")
        dev = self.__dict__.get("_pal_dev")
        if dev is None or dev.device != torch.device(device):
            dev = self.__dict__["_pal_dev"] = torch.from_numpy(np.ascontiguousarray(self.PALETTE)).to(device)
        return dev

    def extract_feat(self, img):
        return self.backbone.forward_rows(img)

    def encode_decode_rows(self, img):
        """img fp32 [B, 3, H, W] normalised -> (logits fp32 rows [B*h*w, ld], h, w) at stride 4, BEFORE encode_decode's resize (ops.seg_argmax
        composes it with whole_inference's)."""
        return self.decode_head.forward_rows(self.extract_feat(img), img.shape[0])

    def _two(self, shape):
        shape = tuple(int(v) for v in shape)[:2]
        if len(shape) != 2:
            raise ValueError(f"EncoderDecoder: ori_shape must be (height, width[, 3]), got {shape}")
        return shape

    def simple_test(self, img, ori_shape=None, flip=False, want_colours=False):
        """simple_test with rescale=True on a batch that shares one `ori_shape` (default: the input's size): uint8 labels [B, Ho, Wo]; with
        `want_colours` (labels, palette[label] uint8 [B, Ho, Wo, 3])."""
        if flip:
            raise NotImplementedError("EncoderDecoder: flipped inference is not built")
        rows, h, w = self.encode_decode_rows(img)
        B, _, H, W = img.shape
        out = self._two(ori_shape) if ori_shape is not None else (H, W)
        pal = self._palette_on(img.device) if want_colours else None
        return ops.seg_argmax(rows, self.num_classes, B, h, w, (H, W), out, palette=pal)

    def aug_test(self, *a, **k):
        raise NotImplementedError("EncoderDecoder: aug_test (multi-scale / flip test-time augmentation) is not built")

    def slide_inference(self, *a, **k):
        raise NotImplementedError("EncoderDecoder: slide inference is not built (whole-image inference only)")

    def preprocess(self, bgr, device=None):
        """inference_segmentor's test pipeline on one uint8 BGR image [H, W, 3] (numpy or tensor): keep-ratio rescale to img_scale (2048, 512) with
        `rescale_size`'s arithmetic (bilinear through torch, half-pixel centres, rounded back to the 0 .. 255 integers as a uint8 resize returns them;
        not compared with cv2.resize, which is not a dependency here; a 512x512 image is not resized at all), BGR -> RGB, normalisation, no padding.
        Returns (fp32 [1, 3, h, w], ori_shape)."""
        t = torch.as_tensor(np.ascontiguousarray(bgr) if isinstance(bgr, np.ndarray) else bgr)
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise TypeError(f"EncoderDecoder: expected a uint8 BGR image [H, W, 3], got {t.dtype} {tuple(t.shape)}")
        device = device or next(self.parameters()).device
        H, W = t.shape[:2]
        nw, nh = rescale_size((W, H), IMG_SCALE)
        x = t.to(device).permute(2, 0, 1).float().unsqueeze(0)
        if (nh, nw) != (H, W):
            x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False).round_().clamp_(0, 255)
        x = x.flip(1)                                                                              # BGR -> RGB (to_rgb=True)
        mean = torch.tensor(IMG_MEAN, device=device).view(1, 3, 1, 1)
        std = torch.tensor(IMG_STD, device=device).view(1, 3, 1, 1)
        return ((x - mean) / std).contiguous(), (H, W)

    def colour_image(self, bgr):
        """One uint8 BGR image [H, W, 3] -> uint8 [H, W, 3] numpy = PALETTE[label] in the palette's own (RGB) order, as show_result_pyplot returns it
        with opacity=1."""
        x, ori = self.preprocess(bgr)
        _, colours = self.simple_test(x, ori, want_colours=True)
        return colours[0].cpu().numpy()

    def forward(self, img, ori_shape=None):
        return self.simple_test(img, ori_shape)
