"""Fixture generator for the UPerNet head and the segment map: tests/golden/upernet_tiny_{w,io}.npz, ade_palette.npz.

Runs on a development machine only: it imports the reference's own vendored `uniformer` package (pass the reference checkout with --reference or
ANYEDIT_REFERENCE; nothing of it is copied into this tree) through a made-up top-level module named `uniformer` whose `__path__` is the reference's
`AnyEdit_Collection/other_modules/uniformer` directory, behind inert `sys.modules` stubs for the foreign libraries that package imports and this
run never calls (cv2, torchvision, addict, yapf, terminaltables, prettytable, mmcv, timm: each stubbed only if it cannot be imported).  It runs the
reference's `UPerHead`, `EncoderDecoder.simple_test` / `show_result` (borrowed by a small nn.Module whose `extract_feat` returns the stored backbone
maps), `get_palette('ade')` and `rescale_size`, on the CPU.  The tests read only the .npz files.  Chain of trust: the reference produces the stored
logits and labels -> tests/upernet_ref.py, a plain-torch restatement, is pinned to them by the CPU suite -> the GPU suite trusts the restatement at
the UniFormer-S widths, which no fixture could hold.

Geometry: UPerHead(in_channels=[16, 32, 64, 64], channels=32, num_classes=150, pool_scales=(1, 2, 3, 6), norm_cfg=BN), eval mode, on the four maps
stored in uniformer_tiny_io.npz for the 2x64x48, 1x72x56 (last map 2x1: the pools of 3 and 6 repeat pixels) and 1x40x104 images.  Weights from
upernet_ref.seeded_head_state_dict, loaded strictly.

Fixture conditions, asserted here and re-checked by the CPU suite, per image; seeds are tried in order from upernet_ref.TINY_SEED:
  * the bf16-storage control's rel-L2 on the stride-4 logits lies in uniformer_ref.FIXTURE_BAND;
  * at least 8 distinct labels occur;
  * with e_ctl the control's largest absolute error on the resized logits, at most 40 % of the pixels have a top-two margin below 3 e_ctl;
  * the number of pixels where argmax(softmax(x)) != argmax(x) is recorded (`softmax_flips.*`).

Files (each below the repository's 1 MiB limit):
  upernet_tiny_w.npz   w.<key>: the head's state dict (int16 = bf16 bits for the matrices drawn as bf16 values, float32 / int64 otherwise)
  upernet_tiny_io.npz  logits.<name> fp32 [B, 150, h, w]; labels.<name>.<Ho>x<Wo> uint8 [B, Ho, Wo] for ori_shape = the input's size and for a second
                       one the input does not divide; colour.<name> uint8 [Ho, Wo, 3] = show_result_pyplot's array for image 0 at the input's size;
                       margin.<name>.<Ho>x<Wo> fp16-safe fp32 top-two margins of the reference's resized logits; softmax_flips.<name>.<Ho>x<Wo>;
                       rescale.table int64 [n, 4] = (w, h, new w, new h) of rescale_size((w, h), (2048, 512))
  ade_palette.npz      palette uint8 [150, 3] = get_palette('ade'); classes: the 150 names
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

FOREIGN = ("cv2", "torchvision", "addict", "yapf", "terminaltables", "prettytable", "mmcv", "timm")
RESCALE_SIZES = [(512, 512), (640, 480), (480, 640), (1024, 768), (500, 375), (333, 500), (4000, 300), (300, 4000), (2048, 512), (100, 100), (513, 511),
                 (1920, 1080), (37, 53)]


class _Stub(types.ModuleType):
    """a module every attribute of which is an inert class (usable as a base class, a decorator or a constant) or a sub-stub"""
    __version__ = "9.9.9"
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        value = type(name, (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, *a, **k: (a[0] if a else None)})
        setattr(self, name, value)
        return value


class _StubFinder:
    """resolves `import stubbed.sub.module` for the stubbed top-level names"""

    def __init__(self, names):
        self.names = names

    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in self.names:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def load_reference(root):
    missing = []
    for name in FOREIGN:
        try:
            importlib.import_module(name)
        except ImportError:
            missing.append(name)
    sys.meta_path.insert(0, _StubFinder(tuple(missing)))
    if "timm" in missing:
        layers = importlib.import_module("timm.models.layers")
        layers.DropPath = lambda *a, **k: torch.nn.Identity()
        layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        layers.trunc_normal_ = torch.nn.init.trunc_normal_
    if "addict" in missing:
        importlib.import_module("addict").Dict = dict
    pkg = types.ModuleType("uniformer")
    pkg.__path__ = [os.path.join(root, "AnyEdit_Collection", "other_modules", "uniformer")]
    sys.modules["uniformer"] = pkg
    ns = types.SimpleNamespace()
    ns.UPerHead = importlib.import_module("uniformer.mmseg.models.decode_heads.uper_head").UPerHead
    ns.EncoderDecoder = importlib.import_module("uniformer.mmseg.models.segmentors.encoder_decoder").EncoderDecoder
    ev = importlib.import_module("uniformer.mmseg.core.evaluation")
    ns.get_palette, ns.get_classes = ev.get_palette, ev.get_classes
    ns.rescale_size = importlib.import_module("uniformer.mmcv.image.geometric").rescale_size
    return ns


def borrowed_segmentor(ref, head, maps):
    """simple_test and show_result of the reference's EncoderDecoder on a module whose extract_feat returns the stored backbone maps"""
    ED = ref.EncoderDecoder

    class Borrowed(torch.nn.Module):
        _decode_head_forward_test, encode_decode, whole_inference = ED._decode_head_forward_test, ED.encode_decode, ED.whole_inference
        inference, simple_test, show_result = ED.inference, ED.simple_test, ED.show_result

        def __init__(self):
            super().__init__()
            self.decode_head, self.align_corners, self.num_classes = head, head.align_corners, head.num_classes
            self.test_cfg = types.SimpleNamespace(mode="whole")
            self.CLASSES, self.PALETTE = ref.get_classes("ade"), ref.get_palette("ade")

        def extract_feat(self, img):
            return maps

    return Borrowed().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    ap.add_argument("--seeds", type=int, default=20, help="how many seeds to try from upernet_ref.TINY_SEED on")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    ref = load_reference(args.reference)
    import uniformer_ref as UR
    import upernet_ref as R
    bio = np.load(os.path.join(OUT, "uniformer_tiny_io.npz"))
    geo = R.TINY_HEAD
    head = ref.UPerHead(in_channels=list(geo["in_channels"]), in_index=[0, 1, 2, 3], channels=geo["channels"], num_classes=geo["num_classes"],
                        pool_scales=geo["pool_scales"], dropout_ratio=0.1, norm_cfg=dict(type="BN", requires_grad=True), align_corners=False).float().eval()
    palette = np.array(ref.get_palette("ade"), dtype=np.int64)
    assert palette.shape == (150, 3) and palette[:3].tolist() == [[120, 120, 120], [180, 120, 120], [6, 230, 230]] and palette.min() >= 0 and palette.max() <= 255
    lo, hi = UR.FIXTURE_BAND
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    for seed in range(R.TINY_SEED, R.TINY_SEED + args.seeds):
        sd = R.seeded_head_state_dict(seed=seed, **geo)
        head.load_state_dict(sd, strict=True)
        io, ok = {}, True
        for (B, H, W) in UR.TINY_SIZES:
            name = f"{B}x{H}x{W}"
            maps = [torch.from_numpy(bio[f"out.{name}.{k}"]) for k in range(4)]
            img = torch.from_numpy(bio["x." + name])
            with torch.no_grad():
                logits = head(maps)
            mine, ctl = R.head_forward(sd, maps, geo["pool_scales"]), R.head_control(sd, maps, geo["pool_scales"])
            e_ctl = rel(ctl, logits)
            io["logits." + name] = logits.numpy()
            seg = borrowed_segmentor(ref, head, maps)
            line = f"seed {seed} {name}: logits {tuple(logits.shape)} std {float(logits.std()):.2f}; restatement {rel(mine, logits):.1e}; control {e_ctl:.2e}"
            ok &= lo <= e_ctl <= hi
            for ori in ((H, W), R.SECOND_ORI[name]):
                metas = [dict(ori_shape=(ori[0], ori[1], 3), img_shape=(H, W, 3), flip=False)] * B
                with torch.no_grad():
                    labels = np.stack(seg.simple_test(img, metas, rescale=True))
                    full = R.resize_twice(logits, (H, W), ori)
                    full_ctl = R.resize_twice(ctl, (H, W), ori)
                assert np.array_equal(labels, full.softmax(1).argmax(1).numpy()), "simple_test is softmax then argmax of the two resizes"
                flips = int((full.softmax(1).argmax(1) != full.argmax(1)).sum())
                margin = R.top_two_margin(full)
                e_abs = float((full_ctl - full).abs().max())
                near = float((margin < 3 * e_abs).float().mean())
                distinct = len(np.unique(labels))
                key = f"{name}.{ori[0]}x{ori[1]}"
                io["labels." + key] = labels.astype(np.uint8)
                io["margin." + key] = margin.numpy()
                io["softmax_flips." + key] = np.array(flips, dtype=np.int64)
                line += f"; {ori[0]}x{ori[1]}: {distinct} labels, e_ctl {e_abs:.2e}, {100 * near:.1f} % within 3 e_ctl, {flips} softmax flips"
                ok &= distinct >= 8 and near <= 0.40
                if ori == (H, W):
                    shown = seg.show_result(np.zeros((H, W, 3), dtype=np.uint8), [labels[0]], palette=ref.get_palette("ade"), show=False, opacity=1)
                    io["colour." + name] = np.ascontiguousarray(shown[..., ::-1]).astype(np.uint8)          # show_result_pyplot: bgr2rgb
                    assert np.array_equal(io["colour." + name], palette[labels[0]].astype(np.uint8))
            print(line)
        if ok:
            break
        print(f"seed {seed} does not meet the fixture conditions")
    assert ok, f"no seed of {args.seeds} met the fixture conditions"
    print(f"seed chosen: {seed} (upernet_ref.TINY_SEED must name it)")
    assert seed == R.TINY_SEED, "set upernet_ref.TINY_SEED to the seed chosen and run again"
    io["rescale.table"] = np.array([[w, h, *ref.rescale_size((w, h), (2048, 512))] for w, h in RESCALE_SIZES], dtype=np.int64)
    w = {}
    for k, v in sd.items():
        if R.stored_as_bf16(k):
            assert torch.equal(v.bfloat16().float(), v), k
            w["w." + k] = v.bfloat16().view(torch.int16).numpy()
        else:
            w["w." + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "upernet_tiny_w.npz"), **w)
    np.savez_compressed(os.path.join(OUT, "upernet_tiny_io.npz"), **io)
    np.savez_compressed(os.path.join(OUT, "ade_palette.npz"), palette=palette.astype(np.uint8), classes=np.array(ref.get_classes("ade")))
    for f in ("upernet_tiny_w.npz", "upernet_tiny_io.npz", "ade_palette.npz"):
        size = os.path.getsize(os.path.join(OUT, f))
        print(f, size)
        assert size < 1 << 20


if __name__ == "__main__":
    main()
