"""Thin Python operators over the C ABI (include/anyedit_hip.h).  Tensor plumbing only: shape/dtype/contiguity
checks, output allocation, stream lookup.  All arithmetic happens in the HIP kernels; there is no fallback path.

Activations are channels-last bf16: [rows, C] with rows = B*H*W.
"""
import torch

import collections
import ctypes
import os
import threading

from ._lib import lib, check as _check

BF16 = torch.bfloat16
EPI_NONE, EPI_GELU, EPI_GEGLU, EPI_SILU, EPI_RELU = 0, 1, 2, 3, 4


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


_live = threading.local()


def _tmp(t):
    """Keeps a converted temporary (`x.float().contiguous()` ...) alive until the launch it feeds has been enqueued.

    Without this the temporary is freed as soon as `_p` has taken its address, and the NEXT temporary of the same argument
    list gets the same block back from the caching allocator: two arguments of one kernel would alias.  `check`
    releases the references once the launch call has returned — the allocator's stream ordering covers the rest."""
    if t is not None:
        lst = getattr(_live, "t", None)
        if lst is None:
            lst = _live.t = []
        lst.append(t)
    return t


def check(rc, what=""):
    lst = getattr(_live, "t", None)
    if lst:
        lst.clear()
    _check(rc, what)


def weights_token(*tensors):
    """Identity + in-place version of every tensor a packed-weight cache was built from: (storage address, autograd version counter).
    `load_state_dict` (on the module or on ANY parent), torch optimizer steps and `.to(device)` all change it, so a cache keyed on the
    token can never serve stale packed weights (only the outermost load_state_dict used to invalidate).  Kernels that
    update parameters through raw pointers do NOT move the counter by themselves: `AnySDTrainer.optimizer_step` bumps it after
    `adamw_step` (torch.autograd.graph.increment_version), and any other raw-pointer writer must do the same."""
    return tuple((t.data_ptr(), _version_of(t)) for t in tensors if t is not None)


def _version_of(t):
    try:
        return t._version
    except RuntimeError:      # inference tensors carry no version counter: identity only
        return -1


def cache_stale(mod, attr, *tensors):
    """True when `mod.<attr>` is missing or was built from other values of `tensors`; records the new token (the caller rebuilds now)."""
    tok = weights_token(*tensors)
    if getattr(mod, attr, None) is None or mod.__dict__.get(attr + "_tok") != tok:
        mod.__dict__[attr + "_tok"] = tok
        return True
    return False


def _chk(t, dtype, name, dims=None):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a GPU tensor (anyedit_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name}: expected {dims} dims, got shape {tuple(t.shape)}")


def _dense(t, dtype, name, dims=None):
    """`t` as the kernels read it: a GPU tensor of `dtype` (TypeError otherwise), copied if its layout is not row-major contiguous"""
    _chk(t, dtype, name, dims)
    return t.contiguous()


def _target(t, dtype, shape, name):
    """a tensor a kernel writes in place: it must already be contiguous (a copy would not reach the caller)"""
    _chk(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {tuple(shape)} tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


# --------------------------------------------------------------------------- weight packing (host side, once)
def pack_linear(w):
    """nn.Linear / 1x1 conv weight -> bf16 [N, K] contiguous."""
    return w.detach().reshape(w.shape[0], -1).to(BF16).contiguous()


def pack_conv3x3(w, cin_pad=None, k_order=0):
    """[Cout, Cin, 3, 3] -> bf16 [Cout, 9*Cin_pad], K ordered (ky, kx, cin) to match the implicit-GEMM gather; k_order = 1: K ordered
    (cin // 64, ky, kx, cin % 64) — the chunk-major order of `conv3x3(..., k_order=1)` (same values, another column order)."""
    cout, cin = w.shape[0], w.shape[1]
    cin_pad = cin_pad or ((cin + 63) // 64 * 64)
    wp = torch.zeros(cout, 3, 3, cin_pad, dtype=BF16, device=w.device)
    wp[..., :cin] = w.detach().permute(0, 2, 3, 1).to(BF16)
    if k_order == 1:
        wp = wp.reshape(cout, 9, cin_pad // 64, 64).permute(0, 2, 1, 3)
    return wp.reshape(cout, 9 * cin_pad).contiguous()


def pack_conv3x3_taps8(w):
    """[Cout, 8, 3, 3] -> bf16 [Cout, 128], column 8 * (3 ky + kx) + cin, zeros in columns 72..127: the stem conv as a dense GEMM over
    `im2col3x3_c8` rows (same products as the implicit GEMM, a ninth of its K extent)."""
    cout, cin = w.shape[0], w.shape[1]
    assert cin == 8 and tuple(w.shape[2:]) == (3, 3)
    wp = torch.zeros(cout, 128, dtype=BF16, device=w.device)
    wp[:, :72] = w.detach().permute(0, 2, 3, 1).reshape(cout, 72).to(BF16)
    return wp.contiguous()


def pack_conv3x3_up2(w):
    """[Cout, Cin, 3, 3] (fp32 master) -> bf16 [4, Cout, 4*Cin]: the weights of `conv3x3_up2` — nearest-x2 upsampling followed by the 3x3 conv equals, per
    output parity (py, px), a 2x2 conv on the low-resolution input whose taps are SUMS of the 3x3 taps that land on the same input pixel
    (row pairs: py = 0 -> {w[0]}, {w[1] + w[2]}; py = 1 -> {w[0] + w[1]}, {w[2]}; columns likewise).  Summed in fp32, rounded to bf16 once."""
    cout, cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3) and cin % 64 == 0
    return up2_weight_sums(w).reshape(4, cout, 4 * cin).to(BF16).contiguous()


def up2_weight_sums(w):
    """fp32 [4, Cout, 4, Cin]: set 2 py + px, tap 2 i + j of `pack_conv3x3_up2` before the rounding (tests/test_host_logic.py restates the identity on CPU)."""
    cout, cin = w.shape[0], w.shape[1]
    w32 = w.detach().float()
    sets = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    out = torch.empty(4, cout, 4, cin, dtype=torch.float32, device=w.device)
    for py in range(2):
        for px in range(2):
            for i in range(2):
                for j in range(2):
                    acc = torch.zeros(cout, cin, dtype=torch.float32, device=w.device)
                    for ky in sets[(py, i)]:
                        for kx in sets[(px, j)]:
                            acc = acc + w32[:, :, ky, kx]
                    out[2 * py + px, :, 2 * i + j] = acc
    return out


_UP2_SUBPIXEL = os.environ.get("AE_UP2_SUBPIXEL", "1") != "0"  # tuning knob (A/B): 0 = the up-convs through the upsampling gather of ae_conv3x3_bf16 (9 taps per output pixel)


def up2_subpixel_ok(Cin, Cout, H, W, want_stats):
    """True where `Upsample`'s nearest-x2 + conv runs as four 2x2 convs on the low-resolution map (not under the training tape: its conv node and
    adjoint keep the gather form)."""
    return _UP2_SUBPIXEL and Cin % 64 == 0 and Cout % 8 == 0 and (not want_stats or (H * W) % 32 == 0) and not (_TAPE is not None and _TAPE.active)


def conv3x3_up2(x, w4, bias, B, H, W, out=None, colstats=None):
    """conv3x3(nearest_upsample_x2(x)) on channels-last rows: x [B*H*W, Cin] bf16, w4 = `pack_conv3x3_up2(weight)` -> ([B*2H*2W, Cout], 2H, 2W).
    colstats: optional `colstats_buffer(B*4*H*W, Cout)` for the consuming GroupNorm."""
    _chk(x, BF16, "conv3x3_up2.x", 2)
    _chk(w4, BF16, "conv3x3_up2.w4", 3)
    Cin, Cout = x.shape[1], w4.shape[1]
    if x.shape[0] != B * H * W or not x.is_contiguous():
        raise ValueError(f"conv3x3_up2: x must be contiguous [B*H*W, Cin] = [{B * H * W}, Cin], got {tuple(x.shape)}")
    if tuple(w4.shape) != (4, Cout, 4 * Cin) or not w4.is_contiguous():
        raise ValueError(f"conv3x3_up2: packed weight must be a contiguous [4, Cout, {4 * Cin}] tensor, got {tuple(w4.shape)}")
    if out is None:
        out = torch.empty(B * 4 * H * W, Cout, dtype=BF16, device=x.device)
    if colstats is not None:
        _chk(colstats, torch.float32, "conv3x3_up2.colstats", 3)
        if tuple(colstats.shape) != (B * 4 * H * W // 32, Cout, 2) or not colstats.is_contiguous() or (H * W) % 32:
            raise ValueError(f"conv3x3_up2: colstats must be a contiguous [{B * 4 * H * W // 32}, {Cout}, 2] fp32 buffer (H * W % 32 == 0)")
    check(lib.ae_conv3x3_up2_bf16(_p(x), _p(w4), _p(bias), _p(out), B, H, W, Cin, Cout, _p(colstats), _s()), "ae_conv3x3_up2_bf16")
    return out, 2 * H, 2 * W


_STEM_IM2COL = os.environ.get("AE_STEM_IM2COL", "1") != "0"  # tuning knob (A/B): 0 = the stem conv through the implicit-GEMM kernel (Cin = 8 padded to 64 per tap)


def stem_im2col_ok(Cin, stride, upsample2x):
    """True where a 3x3 conv runs as im2col + dense GEMM: the 8-channel stem (not under the training tape, whose conv node keeps the implicit-GEMM form)."""
    return _STEM_IM2COL and Cin == 8 and stride == 1 and not upsample2x and not (_TAPE is not None and _TAPE.active)


def im2col3x3_c8(x, B, H, W):
    """x: [B*H*W, 8] bf16 channels-last -> [B*H*W, 128] bf16 (`pack_conv3x3_taps8` column order)."""
    _chk(x, BF16, "im2col3x3_c8.x", 2)
    if tuple(x.shape) != (B * H * W, 8) or not x.is_contiguous():
        raise ValueError(f"im2col3x3_c8: x must be contiguous [{B * H * W}, 8], got {tuple(x.shape)}")
    y = torch.empty(B * H * W, 128, dtype=BF16, device=x.device)
    check(lib.ae_im2col3x3_c8_bf16(_p(x), _p(y), B, H, W, _s()), "ae_im2col3x3_c8_bf16")
    return y


_CONV_KMAJOR = int(os.environ.get("AE_CONV_KMAJOR", "2"))  # tuning knob: 0 off, 1 un-split 192x320 plan, 2 + its split-K form, 3 every eligible conv, 4 un-split 192x320 and 128x128 plans


# --------------------------------------------------------------------------- launch plans: the library says what it would run
Plan = collections.namedtuple("Plan", "BM BN AMODE WAVES_M WAVES_N GLDS WAVES_K STAGES CS LAB WA XE grid threads lds splitk reduce colstats rowpanel")
_PLANS = {}


def _plan(query, *args):
    """The plan[] of `ae_gemm_plan` / `ae_conv3x3_plan` / `ae_conv3x3_up2_plan` (include/anyedit_hip.h: the library's own launch selection, run
    without launching; host only), cached per argument tuple — the library latches its AE_* knobs once per process, so an answer never changes.
    None: the launch would be refused."""
    key = (query,) + args
    if key not in _PLANS:
        buf = (ctypes.c_int * len(Plan._fields))()
        _PLANS[key] = Plan(*buf) if getattr(lib, query)(*args, buf) == 0 else None
    return _PLANS[key]


def gemm_plan(M, N, K, epilogue=EPI_NONE, Ksplit=0, out_f32=False, colstats=False, ln_mode=0):
    """What `gemm` (ln_mode 0) / `gemm_ln`'s launch (1 emits row statistics, 2 consumes them) would run."""
    return _plan("ae_gemm_plan", M, N, K, epilogue, Ksplit, int(out_f32), int(colstats), ln_mode)


def conv_plan(B, H, W, Cin, Cout, stride=1, upsample2x=0, out_f32=False, colstats=False, k_order=0):
    """What `conv3x3` would run (it always offers the split-K workspace)."""
    return _plan("ae_conv3x3_plan", B, H, W, Cin, Cout, stride, int(upsample2x), int(out_f32), 1, int(colstats), int(k_order))


def up2_plan(B, H, W, Cin, Cout, colstats=False):
    return _plan("ae_conv3x3_up2_plan", B, H, W, Cin, Cout, int(colstats))


def plan_label(p):
    """"192x320", "192x320,splitK", "128x128,ring3", "128x160", ...: tile, three-stage ring, split-K — how the profiler rows name a plan"""
    return f"{p.BM}x{p.BN}" + (",ring3" if p.STAGES == 3 else "") + (",splitK" if p.splitk > 1 else "")


def conv_k_order(M, Cin, Cout, stride=1, upsample2x=False):
    """Which packed K order `conv3x3` should be given for this launch: the chunk-major order where the library plans the 192x320 tile
    (64x64 UNet level at batch >= 12: a block's nine tap windows are then re-read from L2 instead of the MALL), the tap-major order
    elsewhere (measured slower there) and always under the tape (the backward passes use rotated tap-major packs).
    M: output rows.  Tile and split of a conv depend on the map's size only through M, so the question is put for M one-pixel samples."""
    if _CONV_KMAJOR == 0 or upsample2x or Cin % 64 != 0 or (_TAPE is not None and _TAPE.active):
        return 0
    p = conv_plan(M, 1, 1, Cin, Cout, stride)
    if p is None or not p.GLDS:   # the chunk-major order exists in the LDS-DMA loader only
        return 0
    if _CONV_KMAJOR == 3:
        return 1
    label = plan_label(p)
    if _CONV_KMAJOR == 4:   # (A/B only) the un-split plans of the 64x64 and 32x32 levels
        return 1 if label in ("192x320", "128x128") else 0
    return 1 if (label == "192x320" or (_CONV_KMAJOR >= 2 and label == "192x320,splitK")) else 0


def pack_geglu(w, b):
    """GEGLU proj [2*inner, dim]: interleave 16 'a' rows with the matching 16 'gate' rows (AE_EPI_GEGLU layout)."""
    inner = w.shape[0] // 2
    assert inner % 16 == 0
    a, g = w[:inner], w[inner:]
    wp = torch.stack([a.reshape(inner // 16, 16, -1), g.reshape(inner // 16, 16, -1)], dim=1).reshape(2 * inner, -1)
    bp = torch.stack([b[:inner].reshape(-1, 16), b[inner:].reshape(-1, 16)], dim=1).reshape(-1)
    return wp.detach().to(BF16).contiguous(), bp.detach().float().contiguous()


def pack_ff2_fused(w2):
    """ff2 weight [C = 320, H] -> the LDS images of `ae_ff_fused_bf16` (csrc/ff_fused.hip), bf16 [H / 32, C, 32], once per weight version.
    Image row i of a 32-hidden-unit chunk holds output column 32 (i >> 5) + 8 ((i & 15) >> 2) + 4 ((i & 31) >> 4) + (i & 3) (a lane's two result
    fragments are eight consecutive columns: 16-byte stores).  Its 64 bytes are four 16-byte pieces; logical piece g, element e, is hidden unit
    32 s + 16 (e >> 2) + 4 g + (e & 3) — the order the gated values of chunks 2 s, 2 s + 1 sit in the P1 result registers of lane group g —
    stored at position (g + 2 ((i & 15) >> 2)) & 3 (conflict-free ds_read_b128 lane groups)."""
    C, H = w2.shape
    assert C == 320 and H % 32 == 0
    dev = w2.device
    i = torch.arange(C, device=dev)
    i5 = i & 31
    col = 32 * (i >> 5) + 8 * ((i5 & 15) >> 2) + 4 * (i5 >> 4) + (i5 & 3)
    pos = torch.arange(4, device=dev)
    e = torch.arange(8, device=dev)
    gp = (pos[None, :] - 2 * ((i[:, None] & 15) >> 2)) & 3                                         # [C, 4]: the logical piece stored at (row, position)
    u = 16 * (e >> 2)[None, None, :] + 4 * gp[:, :, None] + (e & 3)[None, None, :]                  # [C, 4, 8] hidden unit inside the chunk
    wf = w2.detach().float()[col]                                                                  # rows in image order
    img = wf.reshape(C, H // 32, 32).permute(1, 0, 2)                                              # [S, C, 32]
    idx = u.reshape(1, C, 32).expand(H // 32, C, 32)
    return torch.gather(img, 2, idx).to(BF16).contiguous()


def ff_fused_ok(M, C, H):
    """True where `ff_fused` covers the feed-forward shape (never while the training tape records: its backward needs the pre-activations)."""
    return not (_TAPE is not None and _TAPE.active) and bool(lib.ae_ff_fused_supported(M, C, H))


def ff_fused(x, gamma, beta, eps, w1, b1, w2img, b2, residual=None, out=None, w3=None, b3=None, residual3=None, colstats=None):
    """out = FF(LayerNorm(x)) (+ residual) in ONE launch (attention.py:49-76 behind norm3, :271-275): x [M, 320] bf16 rows, (w1, b1) = `pack_geglu`,
    w2img = `pack_ff2_fused`.  With w3 (bf16 [320, 320], `pack_linear`): out = bf16(that) @ w3^T + b3 (+ residual3) — SpatialTransformer.proj_out and its
    residual (attention.py:337-340) in the same launch; colstats: `colstats_buffer(M, 320)` for the GroupNorm that consumes out.  Callers ask `ff_fused_ok` first."""
    _chk(x, BF16, "ff_fused.x", 2)
    _chk(w1, BF16, "ff_fused.w1", 2)
    _chk(w2img, BF16, "ff_fused.w2img", 3)
    _chk(gamma, torch.float32, "ff_fused.gamma", 1)
    _chk(beta, torch.float32, "ff_fused.beta", 1)
    _chk(b1, torch.float32, "ff_fused.b1", 1)
    M, C = x.shape
    H = w1.shape[0] // 2
    if w1.shape[1] != C or tuple(w2img.shape) != (H // 32, C, 32) or not w2img.is_contiguous() or x.stride(1) != 1 or w1.stride(1) != 1:
        raise ValueError(f"ff_fused: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, w2img {tuple(w2img.shape)} do not fit together")
    if b1.numel() != 2 * H or gamma.numel() != C or beta.numel() != C:
        raise ValueError("ff_fused: b1 / gamma / beta sizes")
    if b2 is not None:
        _chk(b2, torch.float32, "ff_fused.b2", 1)
    if residual is not None:
        _chk(residual, BF16, "ff_fused.residual", 2)
    if w3 is not None:
        _chk(w3, BF16, "ff_fused.w3", 2)
        if tuple(w3.shape) != (C, C) or w3.stride(1) != 1:
            raise ValueError("ff_fused: w3 must be [C, C] with unit inner stride")
        if b3 is not None:
            _chk(b3, torch.float32, "ff_fused.b3", 1)
        if residual3 is not None:
            _chk(residual3, BF16, "ff_fused.residual3", 2)
        if colstats is not None:
            _chk(colstats, torch.float32, "ff_fused.colstats", 3)
            if tuple(colstats.shape) != ((M + 31) // 32, C, 2) or not colstats.is_contiguous():
                raise ValueError(f"ff_fused: colstats must be a contiguous [{(M + 31) // 32}, {C}, 2] fp32 buffer")
    elif b3 is not None or residual3 is not None or colstats is not None:
        raise ValueError("ff_fused: b3 / residual3 / colstats go with w3")
    if out is None:
        out = torch.empty(M, C, dtype=BF16, device=x.device)
    _chk(out, BF16, "ff_fused.out", 2)
    check(lib.ae_ff_fused_bf16(_p(x), x.stride(0), _p(gamma), _p(beta), float(eps), _p(w1), w1.stride(0), _p(b1), _p(w2img), _p(b2), _p(residual),
                               residual.stride(0) if residual is not None else 0, _p(w3), w3.stride(0) if w3 is not None else 0, _p(b3), _p(residual3),
                               residual3.stride(0) if residual3 is not None else 0, _p(colstats), _p(out), out.stride(0), M, C, H, _s()), "ae_ff_fused_bf16")
    return out


# --------------------------------------------------------------------------- GEMM / conv
def colstats_buffer(M, N, device):
    """fp32 [ceil(M/32), N, 2]: per-channel (sum, sum of squares) over each 32-row slab of a bf16 [M, N] activation — filled by the kernel
    that PRODUCES the activation (`colstats=` of gemm / ln_gemm / conv3x3) and consumed by `groupnorm(..., colstats=...)`, which then
    skips its own statistics pass (the GroupNorm inputs of the 64x64 / 32x32 UNet levels: SURVEY.md §7 hard part (iii))."""
    return torch.empty((M + 31) // 32, N, 2, dtype=torch.float32, device=device)


_GN_COLSTATS = os.environ.get("AE_GN_COLSTATS", "1") != "0"  # tuning knob: 0 = GroupNorm computes its own statistics everywhere (A/B)


def want_colstats(HW):
    """True where a GroupNorm over HW positions per sample takes its statistics from the producer: maps above the single-launch slab
    kernel's range (HW > 256) whose samples are whole 32-row slabs; never while the training tape records (its GroupNorm keeps
    (mean, rstd) for the backward pass through the plain path)."""
    return _GN_COLSTATS and HW > 256 and HW % 32 == 0 and not (_TAPE is not None and _TAPE.active)


def gemm(a, w, bias=None, residual=None, addvec=None, rows_per_batch=0, epilogue=EPI_NONE, out_f32=False, a2=None, out=None, colstats=None,
         rowstats=None):
    """out[M,N] = epi(cat([a, a2], 1) @ w^T).  a: [M,K1] bf16 (row stride free), w: [N,K] bf16.
    colstats: optional `colstats_buffer(M, N)` that receives the per-channel slab statistics of the output.
    rowstats: optional `rowstats_buffer(M, N)` that receives the per-row statistics of the output for the LayerNorm folded into the
    GEMM that consumes it (`gemm_ln`); only where `ln_fold_plan(M, N, K, EPI_NONE, 1)` says the tile plan carries that epilogue."""
    if rowstats is not None:
        if _TAPE is not None and _TAPE.active:
            raise ValueError("gemm: row statistics are not recorded on the training tape (ln_fold_plan is False while it records)")
        if addvec is not None or a2 is not None or out_f32 or colstats is not None or epilogue != EPI_NONE:
            raise ValueError("gemm: rowstats goes with a plain bf16 GEMM (+bias, +residual) only")
        return _gemm_ln(a, w, bias, residual, EPI_NONE, out, rowstats, None, None, 0.0)
    if _TAPE is not None and _TAPE.active:
        return _TAPE.gemm(a, w, bias=bias, residual=residual, addvec=addvec, rows_per_batch=rows_per_batch, epilogue=epilogue, out_f32=out_f32, a2=a2, out=out)
    _chk(a, BF16, "gemm.a", 2)
    _chk(w, BF16, "gemm.w", 2)
    M, K1 = a.shape
    N, K = w.shape
    if a.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("gemm: a and w must have unit inner stride")
    K2 = 0
    if a2 is not None:
        _chk(a2, BF16, "gemm.a2", 2)
        K2 = a2.shape[1]
        if a2.shape[0] != M or a2.stride(1) != 1:
            raise ValueError("gemm: a2 shape mismatch")
    if K1 + K2 != K:
        raise ValueError(f"gemm: K mismatch: a has {K1}+{K2} columns, w has {K}")
    n_out = N // 2 if epilogue == EPI_GEGLU else N
    if out is None:
        out = torch.empty(M, n_out, dtype=torch.float32 if out_f32 else BF16, device=a.device)
    if bias is not None:
        _chk(bias, torch.float32, "gemm.bias", 1)
    if residual is not None:
        _chk(residual, BF16, "gemm.residual", 2)
    if addvec is not None:
        _chk(addvec, torch.float32, "gemm.addvec", 2)
    if colstats is not None:
        _chk(colstats, torch.float32, "gemm.colstats", 3)
        if tuple(colstats.shape) != ((M + 31) // 32, n_out, 2) or not colstats.is_contiguous():
            raise ValueError(f"gemm: colstats must be a contiguous [{(M + 31) // 32}, {n_out}, 2] fp32 buffer")
    if a2 is None and addvec is None and not out_f32 and _rowpanel_ok(a, w, out, residual, M, N, K, epilogue):
        return _ln_gemm_launch(a, w, bias, residual, None, None, 0.0, epilogue, out, M, N, K, colstats)
    check(lib.ae_gemm_bf16(_p(a), a.stride(0), _p(a2), a2.stride(0) if a2 is not None else 0, K1, _p(w), w.stride(0),
                           _p(out), out.stride(0), M, N, K, _p(bias), _p(residual),
                           residual.stride(0) if residual is not None else 0, _p(addvec),
                           addvec.stride(0) if addvec is not None else 0, rows_per_batch, epilogue,
                           1 if out_f32 else 0, _p(colstats), _s()), "ae_gemm_bf16")
    return out


# --------------------------------------------------------------------------- LayerNorm folded into the consuming GEMM
_LN_FOLD = os.environ.get("AE_LN_FOLD", "1") != "0"  # tuning knob (A/B): 0 = a LayerNorm launch in front of every K = 640 / 1280 projection


def ln_fold_plan(M, N, K, epilogue, mode):
    """True where the tile plan `gemm` takes for [M, K] x [N, K]^T carries the row-statistics epilogue (mode 1: this GEMM PRODUCES the
    rows a LayerNorm reads) or the LayerNorm-fold epilogue (mode 2: this GEMM CONSUMES the LayerNorm) — `gemm_plan`, cached per
    shape.  Never while the training tape records (its LayerNorm keeps what the backward pass needs)."""
    if not _LN_FOLD or (_TAPE is not None and _TAPE.active):
        return False
    # shapes of the row-panel kernel (K = 320, the 64x64 level): round 5 gave that kernel the fold forms too (the plan says where they take the
    # launch); no fold there with the row-panel kernel switched off (AE_GEMM_ROWPANEL=0, A/B)
    p = gemm_plan(M, N, K, epilogue, ln_mode=mode)
    return p is not None and (_ROWPANEL or not p.rowpanel)


def rowstats_buffer(M, N, device):
    """fp32 [M, N / 64, 2]: (sum, sum of squares) of every row of a bf16 [M, N] activation over each 64-column slice — filled by the GEMM
    that PRODUCES the activation (`gemm(..., rowstats=)`), consumed by `gemm_ln`."""
    return torch.empty(M, N // 64, 2, dtype=torch.float32, device=device)


def pack_ln_fold(w, bias, gamma, beta, geglu=False):
    """Folds LayerNorm's affine part into the projection behind it (attention.py:271-275): LN(x) W^T + b = rstd (x W'^T - mu s) + c.
    Returns (W' = W diag(gamma) as bf16 [N, K] (GEGLU: rows interleaved as `pack_geglu` does), s = row sums of the bf16 W' — exactly what
    the MFMA multiplies —, c = W beta + b), s and c fp32 [N] in the packed row order.  Once per weight version (host side)."""
    wf = w.detach().float().reshape(w.shape[0], -1).contiguous()
    g, be = gamma.detach().float(), beta.detach().float()
    c = linear_f32(be[None, :].contiguous(), wf, bias)[0]
    wp = wf * g[None, :]
    if geglu:
        wq, c = pack_geglu(wp, c)
    else:
        wq = wp.to(BF16).contiguous()
    s = linear_f32(torch.ones(1, wq.shape[1], dtype=torch.float32, device=wq.device), wq.float())[0]
    return wq, s.contiguous(), c.contiguous()


def _gemm_ln(a, w, bias, residual, epilogue, out, rowstats_out, ln_stats, ln_colsum, eps):
    _chk(a, BF16, "gemm_ln.a", 2)
    _chk(w, BF16, "gemm_ln.w", 2)
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or a.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError(f"gemm_ln: a is [{M}, {K}], w is {tuple(w.shape)}; both need unit inner stride")
    n_out = N // 2 if epilogue == EPI_GEGLU else N
    if out is None:
        out = torch.empty(M, n_out, dtype=BF16, device=a.device)
    _chk(out, BF16, "gemm_ln.out", 2)
    if bias is not None:
        _chk(bias, torch.float32, "gemm_ln.bias", 1)
    if residual is not None:
        _chk(residual, BF16, "gemm_ln.residual", 2)
    nparts = 0
    if rowstats_out is not None:
        if rowstats_out.dtype != torch.float32 or tuple(rowstats_out.shape) != (M, N // 64, 2) or not rowstats_out.is_contiguous():
            raise ValueError(f"gemm: rowstats must be a contiguous fp32 [{M}, {N // 64}, 2] buffer (rowstats_buffer)")
    else:
        if ln_stats.dtype != torch.float32 or ln_stats.dim() != 3 or ln_stats.shape[0] != M or ln_stats.shape[2] != 2 or not ln_stats.is_contiguous() \
                or ln_stats.shape[1] * 64 != K:
            raise ValueError(f"gemm_ln: statistics must be the producer's contiguous fp32 [{M}, {K // 64}, 2] buffer, got {tuple(ln_stats.shape)}")
        _chk(ln_colsum, torch.float32, "gemm_ln.s", 1)
        if bias is None or bias.numel() != N or ln_colsum.numel() != N:
            raise ValueError("gemm_ln: s and c must be fp32 [N]")
        nparts = ln_stats.shape[1]
    return _gemm_ln_launch(a, w, bias, residual, epilogue, out, M, N, K, rowstats_out, ln_stats, nparts, ln_colsum, float(eps))


def _gemm_ln_launch(a, w, bias, residual, epilogue, out, M, N, K, rowstats_out, ln_stats, nparts, ln_colsum, eps):
    check(lib.ae_gemm_ln_bf16(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K, _p(bias), _p(residual),
                              residual.stride(0) if residual is not None else 0, epilogue, _p(rowstats_out), _p(ln_stats), nparts,
                              _p(ln_colsum), eps, _s()), "ae_gemm_ln_bf16")
    return out


def gemm_ln(x, rowstats, wq, s, c, eps, residual=None, epilogue=EPI_NONE, out=None):
    """out = epi(LayerNorm(x) @ w^T + b (+ residual)) with the LayerNorm folded away: x are the UN-normalised rows, `rowstats` their
    statistics from the GEMM that produced them, (wq, s, c) = `pack_ln_fold(w, b, gamma, beta)`.  Callers ask `ln_fold_plan(M, N, K,
    epilogue, 2)` first and keep `ln_gemm` where it says no."""
    return _gemm_ln(x, wq, c, residual, epilogue, out, None, rowstats, s, eps)


_ROWPANEL = os.environ.get("AE_GEMM_ROWPANEL", "1") != "0"  # tuning knob: 0 = tiled kernel only (A/B)


def _rowpanel_ok(a, w, out, residual, M, N, K, epilogue):
    if not _ROWPANEL or not lib.ae_ln_gemm_supported(M, N, K, epilogue):
        return False
    ts = [a, w, out] + ([residual] if residual is not None else [])
    # the row-panel kernel addresses A, C and the residual with 32-bit byte offsets (buffer descriptors, per-block base offsets): shapes
    # whose rows x stride reach 2 GiB fall back to the tiled kernel instead of wrapping
    ld_max = max(t.stride(0) for t in ts if t is not w)
    return all(t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) == 1 for t in ts) and N * w.stride(0) * 2 < 2 ** 31 \
        and (M + 192) * ld_max * 2 < 2 ** 31


def _ln_gemm_launch(a, w, bias, residual, gamma, beta, eps, epilogue, out, M, N, K, colstats=None):
    check(lib.ae_ln_gemm_bf16(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K, _p(bias), _p(residual),
                              residual.stride(0) if residual is not None else 0, _p(gamma), _p(beta), float(eps), epilogue,
                              _p(colstats), _s()),
          "ae_ln_gemm_bf16")
    return out


def ln_gemm(x, gamma, beta, eps, w, bias=None, residual=None, epilogue=EPI_NONE, out=None, colstats=None):
    """out = epi(LayerNorm(x; gamma, beta, eps) @ w^T + bias (+ residual)) — attention.py:271-275's norm -> projection pairs in one
    launch (the normalised rows never go to HBM).  Falls back to layernorm + gemm where the fused kernel does not cover the shape
    and while the training tape records."""
    if not (_TAPE is not None and _TAPE.active):
        _chk(x, BF16, "ln_gemm.x", 2)
        _chk(w, BF16, "ln_gemm.w", 2)
        M, K = x.shape
        N = w.shape[0]
        if w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1:
            n_out = N // 2 if epilogue == EPI_GEGLU else N
            o = out if out is not None else torch.empty(M, n_out, dtype=BF16, device=x.device)
            if _rowpanel_ok(x, w, o, residual, M, N, K, epilogue):
                _chk(gamma, torch.float32, "ln_gemm.gamma", 1)
                _chk(beta, torch.float32, "ln_gemm.beta", 1)
                if bias is not None:
                    _chk(bias, torch.float32, "ln_gemm.bias", 1)
                if residual is not None:
                    _chk(residual, BF16, "ln_gemm.residual", 2)
                return _ln_gemm_fused(x, w, bias, residual, gamma, beta, eps, epilogue, o, M, N, K, colstats)
    return gemm(layernorm(x, gamma, beta, eps), w, bias, residual=residual, epilogue=epilogue, out=out, colstats=colstats)


def conv3x3(x, w, bias, B, H, W, addvec=None, residual=None, stride=1, upsample2x=False, out_f32=False, out=None, colstats=None, k_order=0):
    """x: [B*H*W, Cin] bf16 channels-last, w: packed [Cout, 9*Cin] (`pack_conv3x3` with the same k_order).  Returns ([B*Ho*Wo, Cout], Ho, Wo).
    colstats: optional `colstats_buffer(B*Ho*Wo, Cout)` that receives the per-channel slab statistics of the output."""
    if _TAPE is not None and _TAPE.active:
        if k_order:
            raise ValueError("conv3x3: the tape records convolutions on tap-major packed weights (k_order=0)")
        return _TAPE.conv3x3(x, w, bias, B, H, W, addvec=addvec, residual=residual, stride=stride, upsample2x=upsample2x, out_f32=out_f32, out=out)
    _chk(x, BF16, "conv3x3.x", 2)
    _chk(w, BF16, "conv3x3.w", 2)
    Cin = x.shape[1]
    Cout = w.shape[0]
    if x.shape[0] != B * H * W or not x.is_contiguous():
        raise ValueError(f"conv3x3: x must be contiguous [B*H*W, Cin] = [{B * H * W}, Cin], got {tuple(x.shape)}")
    if w.shape[1] != 9 * ((Cin + 63) // 64 * 64):
        raise ValueError(f"conv3x3: packed weight has K={w.shape[1]}, expected {9 * ((Cin + 63) // 64 * 64)}")
    Hv, Wv = (2 * H, 2 * W) if upsample2x else (H, W)
    Ho, Wo = (Hv - 1) // stride + 1, (Wv - 1) // stride + 1
    if out is None:
        out = torch.empty(B * Ho * Wo, Cout, dtype=torch.float32 if out_f32 else BF16, device=x.device)
    if residual is not None:
        _chk(residual, BF16, "conv3x3.residual", 2)
        if residual.shape != (B * Ho * Wo, Cout) or not residual.is_contiguous():
            raise ValueError("conv3x3: residual shape mismatch")
    nws = lib.ae_conv3x3_workspace_floats(B, H, W, Cin, Cout, stride, int(upsample2x))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws > 0 else None  # split-K partials (small-M layers)
    if colstats is not None:
        _chk(colstats, torch.float32, "conv3x3.colstats", 3)
        if tuple(colstats.shape) != ((B * Ho * Wo + 31) // 32, Cout, 2) or not colstats.is_contiguous():
            raise ValueError(f"conv3x3: colstats must be a contiguous [{(B * Ho * Wo + 31) // 32}, {Cout}, 2] fp32 buffer")
    check(lib.ae_conv3x3_bf16(_p(x), _p(w), _p(bias), _p(addvec), addvec.stride(0) if addvec is not None else 0, _p(residual),
                              _p(out), B, H, W, Cin, Cout, stride, int(upsample2x), 1 if out_f32 else 0, _p(ws), _p(colstats), int(k_order), _s()),
          "ae_conv3x3_bf16")
    return out, Ho, Wo


# --------------------------------------------------------------------------- norms
_GN_COUNTERS = {}


_GN_TAIL = os.environ.get("AE_GN_TAIL") == "1"   # the last-block finalize is a measured loss on MI355X: opt-in only


def _gn_counters(device, B):
    """int32 tickets for the last-block statistics fold (zero between launches), or None while that variant is off.  One buffer per
    (device, stream): launches on a stream are ordered, so they can share it."""
    if not _GN_TAIL:
        return None
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    c = _GN_COUNTERS.get(key)
    if c is None or c.numel() < B:
        c = _GN_COUNTERS[key] = torch.zeros(max(B, 256), dtype=torch.int32, device=device)
    return c


def groupnorm(x, gamma, beta, B, HW, eps, silu=False, groups=32, x2=None, out=None, stat_out=None, colstats=None, colstats2=None):
    """GroupNorm(+SiLU) over channels-last [B*HW, C]; x2: optional second tensor concatenated along channels.
    stat_out: optional fp32 [B, groups, 2] that receives (mean, rstd) for `groupnorm_bwd`.
    colstats / colstats2: per-channel slab statistics of x / x2 from the kernels that produced them (`colstats_buffer`): the statistics
    pass over the activation is skipped.  Both or neither for a two-source input."""
    if _TAPE is not None and _TAPE.active:
        return _TAPE.groupnorm(x, gamma, beta, B, HW, eps, silu=silu, groups=groups, x2=x2, out=out)
    _chk(x, BF16, "groupnorm.x", 2)
    C1 = x.shape[1]
    C = C1 + (x2.shape[1] if x2 is not None else 0)
    if not x.is_contiguous() or (x2 is not None and not x2.is_contiguous()):
        raise ValueError("groupnorm: inputs must be contiguous")
    if out is None:
        out = torch.empty(B * HW, C, dtype=BF16, device=x.device)
    if colstats is not None and (x2 is None) != (colstats2 is None):
        colstats = colstats2 = None   # statistics of only one of the two sources: fall back to the kernel's own pass
    if colstats is not None:
        for t, c, n in ((colstats, C1, "colstats"), (colstats2, C - C1, "colstats2")):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (B * HW // 32, c, 2) or not t.is_contiguous() or HW % 32):
                raise ValueError(f"groupnorm: {n} must be a contiguous fp32 [{B * HW // 32}, {c}, 2] buffer (HW % 32 == 0), got {tuple(t.shape)}")
    nws = int(lib.ae_groupnorm_workspace_floats(B, HW, C, groups))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device)
    check(lib.ae_groupnorm_nhwc_bf16(_p(x), _p(x2), C1, _p(gamma), _p(beta), _p(out), B, HW, C, groups, eps,
                                     1 if silu else 0, _p(ws), _p(_gn_counters(x.device, B)), _p(stat_out), _p(colstats), _p(colstats2), _s()),
          "ae_groupnorm_nhwc_bf16")
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    if _TAPE is not None and _TAPE.active:
        return _TAPE.layernorm(x, gamma, beta, eps=eps, out=out)
    _chk(x, BF16, "layernorm.x", 2)
    if not x.is_contiguous():
        raise ValueError("layernorm: x must be contiguous")
    M, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.ae_layernorm_bf16(_p(x), _p(gamma), _p(beta), _p(out), M, C, eps, _s()), "ae_layernorm_bf16")
    return out


# --------------------------------------------------------------------------- attention
def attention(q, k, v, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, out=None, rel_h=None, rel_w=None,
              kH=0, kW=0, key_mask=None, out_scale=None, accumulate=False, seg2=None, lse=None, lse2=None, o_strides=None):
    """q/k/v: bf16 tensors (any shape) addressed via (batch, head, row) element strides; out: [B, Nq, H*D] bf16, or any bf16 buffer
    addressed through o_strides = (batch, head, row) element strides (multiples of 4).
    seg2 = (k2, v2, Nk2, k2_strides, v2_strides, scale2 [B] fp32): second key/value segment with its own softmax.
    lse / lse2: optional contiguous fp32 [B, H, Nq] outputs kept for attention_bwd: the log2-domain log-sum-exp of each segment's own
    logits, log2 sum_j exp(scale q.k_j [+ bias]).  They do not depend on out_scale, scale2 or accumulate (those act on the output only)."""
    if _TAPE is not None and _TAPE.active:
        return _TAPE.attention(q, k, v, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, out=out, key_mask=key_mask,
                               out_scale=out_scale, accumulate=accumulate, seg2=seg2, rel_h=rel_h)
    if out is None:
        out = torch.empty(B, Nq, H * D, dtype=BF16, device=q.device)
    if o_strides is None:
        o_strides = (Nq * H * D, D, H * D)
    if seg2 is not None:
        k2, v2, Nk2, k2_strides, v2_strides, scale2 = seg2
        seg_args = (_p(k2), _p(v2), Nk2, *k2_strides, *v2_strides, _p(scale2))
    else:
        seg_args = (None, None, 0, 0, 0, 0, 0, 0, 0, None)
    check(lib.ae_attn_fwd_bf16(_p(q), _p(k), _p(v), _p(out), B, H, Nq, Nk, D, *q_strides, *k_strides, *v_strides, *o_strides,
                               scale, _p(rel_h), _p(rel_w), kH, kW, _p(key_mask), _p(out_scale), 1 if accumulate else 0,
                               *seg_args, _p(lse), _p(lse2), _s()), "ae_attn_fwd_bf16")
    return out


_FP8_WS = {}


def attention_fp8(q, k, v, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, out=None, rel_h=None, rel_w=None, kH=0, kW=0):
    """fp8 (e4m3) attention forward (ae_attn_fwd_fp8): same arguments as `attention` for the no-mask / single-segment case; the
    rel-pos bias path needs kW == 64 (SAM global attention).  Accuracy is that of e4m3 operands: rel-L2 ~5e-2 against the fp32
    reference at unit-variance logits (tests/test_hip_ops.py)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, BF16, "attention_fp8." + n)
    if out is None:
        out = torch.empty(B, Nq, H * D, dtype=BF16, device=q.device)
    need = lib.ae_attn_fp8_workspace_bytes(B, H, Nq, Nk, D)
    if need <= 0:
        raise ValueError(f"attention_fp8: unsupported sizes B={B} H={H} Nq={Nq} Nk={Nk} D={D}")
    key = (q.device, torch.cuda.current_stream(q.device).cuda_stream)
    ws = _FP8_WS.get(key)
    if ws is None or ws.numel() < need:  # grow-only scratch per (device, stream): the call owns it until the next call on that stream
        ws = _FP8_WS[key] = torch.empty(need, dtype=torch.uint8, device=q.device)
    if rel_h is not None:
        _chk(rel_h, torch.float32, "attention_fp8.rel_h")
        _chk(rel_w, torch.float32, "attention_fp8.rel_w")
    check(lib.ae_attn_fwd_fp8(_p(q), _p(k), _p(v), _p(out), B, H, Nq, Nk, D, *q_strides, *k_strides, *v_strides, Nq * H * D, D, H * D,
                              float(scale), _p(rel_h), _p(rel_w), kH, kW, _p(ws), ws.numel(), _s()), "ae_attn_fwd_fp8")
    return out


def attention_bwd(q, k, v, dout, lse, B, H, Nq, Nk, D, scale, q_strides, k_strides, v_strides, dq, dk, dv, dq_strides,
                  dk_strides, dv_strides, out_scale=None, accumulate_dq=False, out=None, split_dkv=True, o_strides=None, delta=None):
    """Gradients of one attention segment (ae_attn_bwd_bf16).  dq/dk/dv: bf16 tensors written through the given element strides
    (dk = dv = None when the key/value side needs no gradient).  out: the forward output [B, Nq, H*D] when it is this segment's alone
    (lets the kernel take delta = rowsum(dout o out) up front).  dout (and out) are [B, Nq, H*D], or addressed through o_strides =
    (batch, head, row) element strides (multiples of 8).  lse: the forward's contiguous fp32 [B, H, Nq] log-sum-exp of this segment.
    Returns delta, contiguous fp32 [B, H, Nq] (written into `delta` when given): rowsum(P o dP) with the un-scaled dout — like lse it
    does not depend on out_scale (the gate scales dq / dk / dv only); summed over heads and rows it is the gradient of out_scale[b]."""
    if delta is None:
        delta = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
    if o_strides is None:
        o_strides = (Nq * H * D, D, H * D)
    zero3 = (0, 0, 0)
    ws = None
    if dk is not None and split_dkv:   # few-key segments (cross-attention): the dK / dV pass cuts its query tiles across blocks through fp32 partials
        nws = lib.ae_attn_bwd_workspace_floats(B, H, Nq, Nk, D)
        if nws > 0:
            ws = torch.empty(nws, dtype=torch.float32, device=q.device)
    check(lib.ae_attn_bwd_bf16(_p(q), _p(k), _p(v), _p(dout), _p(out), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, H, Nq, Nk, D,
                               *q_strides, *k_strides, *v_strides, *o_strides, *dq_strides, *(dk_strides if dk is not None else zero3),
                               *(dv_strides if dv is not None else zero3), scale, _p(out_scale), 1 if accumulate_dq else 0, _p(ws), _s()),
          "ae_attn_bwd_bf16")
    return delta


def attention_bhnd(q, k, v, scale=None, key_mask=None):
    """xformers-style entry: q [BH, Nq, D], k/v [BH, Nk, D] contiguous bf16 -> [BH, Nq, D] (attention.py:222-233)."""
    _chk(q, BF16, "attention.q", 3)
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty(BH, Nq, D, dtype=BF16, device=q.device)
    scale = scale if scale is not None else D ** -0.5
    check(lib.ae_attn_fwd_bf16(_p(q), _p(k), _p(v), _p(out), BH, 1, Nq, Nk, D, Nq * D, 0, D, Nk * D, 0, D, Nk * D, 0, D,
                               Nq * D, 0, D, scale, None, None, 0, 0, _p(key_mask), None, 0, None, None, 0, 0, 0, 0, 0, 0, 0, None, None, None, _s()),
          "ae_attn_fwd_bf16")
    return out


# --------------------------------------------------------------------------- CLIP text tower (csrc/clip_text.hip)
ACT_QUICK_GELU, ACT_GELU = 0, 1


def _attention_short(name, fn, q, k, v, extra, B, H, N, D, scale, q_strides, k_strides, v_strides, out, max_n=None, dims=None):
    """The part the three `attention_*_short` wrappers share.  extra: None, or (tensor, dtype, label, shape) of the mask / spans argument, which
    the entry point `fn` takes behind v.  max_n / dims: the N and D ranges to refuse here (None: left to the entry point)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, BF16, f"{name}.{n}")
    if max_n is not None and not 1 <= N <= max_n:
        raise ValueError(f"{name}: sequence length {N}; {fn.__name__} takes between 1 and {max_n}")
    if dims is not None and D not in dims:
        raise ValueError(f"{name}: head_dim {D} is not built (supported: {', '.join(map(str, dims))})")
    ptrs = [_p(q), _p(k), _p(v)]
    if extra is not None:
        t, dtype, label, shape = extra
        _chk(t, dtype, f"{name}.{label}", 3)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: {label} must be a contiguous {list(shape)} tensor, got {tuple(t.shape)}")
        ptrs.append(_p(t))
    if out is None:
        out = torch.empty(B, N, H * D, dtype=BF16, device=q.device)
    _chk(out, BF16, f"{name}.out")
    if out.numel() != B * N * H * D or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous [{B}, {N}, {H * D}] buffer")
    check(fn(*ptrs, _p(out), B, H, N, D, *q_strides, *k_strides, *v_strides, N * H * D, D, H * D, float(scale), _s()), fn.__name__)
    return out


def attention_causal_short(q, k, v, B, H, N, D, scale, q_strides, k_strides, v_strides, out=None):
    """Causal self-attention over at most 128 tokens (the CLIP text tower): q/k/v bf16 tensors addressed through (batch, head, row)
    element strides as in `attention`, out [B, N, H*D] bf16.  Row i attends keys [0, i].  N in [1, 128], D in {32, 64}."""
    return _attention_short("attention_causal_short", lib.ae_attn_causal_short_bf16, q, k, v, None, B, H, N, D, scale, q_strides, k_strides, v_strides, out)


def clip_embed(ids, token_table, position_table, out=None):
    """token_table[ids] + position_table[0:N] -> bf16 rows [B*N, C].  ids: int32 / int64 GPU tensor [B, N]; the tables are bf16 [vocab, C]
    and [positions, C].  The ids are NOT read back to the host (that would be a synchronisation): an id outside [0, vocab) is clamped
    into the table by the kernel.  Range-check ids while they are still on the host (`FrozenCLIPEmbedder.encode_ids` does)."""
    if not ids.is_cuda:
        raise ValueError("clip_embed.ids: expected a GPU tensor (anyedit_amd has no CPU path)")
    if ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 2 or not ids.is_contiguous():
        raise TypeError(f"clip_embed.ids: expected a contiguous int32 / int64 [B, N] tensor, got {ids.dtype} {tuple(ids.shape)}")
    _chk(token_table, BF16, "clip_embed.token_table", 2)
    _chk(position_table, BF16, "clip_embed.position_table", 2)
    B, N = ids.shape
    V, C = token_table.shape
    if position_table.shape[1] != C or not token_table.is_contiguous() or not position_table.is_contiguous():
        raise ValueError("clip_embed: the two tables must be contiguous and of one width")
    if out is None:
        out = torch.empty(B * N, C, dtype=BF16, device=ids.device)
    _chk(out, BF16, "clip_embed.out", 2)
    if tuple(out.shape) != (B * N, C) or not out.is_contiguous():
        raise ValueError(f"clip_embed: out must be a contiguous [{B * N}, {C}] buffer")
    check(lib.ae_clip_embed_bf16(_p(ids), 1 if ids.dtype == torch.int64 else 0, _p(token_table), _p(position_table), _p(out), B, N, C, V,
                                 position_table.shape[0], _s()), "ae_clip_embed_bf16")
    return out


def bias_act(u, bias, act=ACT_QUICK_GELU, out=None):
    """y = act(u + bias) as bf16, u the fp32 [M, N] product of `gemm(..., out_f32=True)`: the pre-activation is never rounded.
    act: ACT_QUICK_GELU (t * sigmoid(1.702 t)) or ACT_GELU (erf)."""
    _chk(u, torch.float32, "bias_act.u", 2)
    _chk(bias, torch.float32, "bias_act.bias", 1)
    M, N = u.shape
    if u.stride(1) != 1 or bias.numel() != N:
        raise ValueError("bias_act: u needs unit inner stride and bias one value per column")
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=u.device)
    _chk(out, BF16, "bias_act.out", 2)
    if tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise ValueError(f"bias_act: out must be [{M}, {N}] with unit inner stride")
    check(lib.ae_bias_act_f32_bf16(_p(u), u.stride(0), _p(bias), _p(out), out.stride(0), M, N, int(act), _s()), "ae_bias_act_f32_bf16")
    return out


def clip_pool_eos(ids, z, eos_token_id, out=None):
    """pooler_output of the CLIP text tower: z[b, first position of eos_token_id in ids[b]] -> [B, C] bf16 (position 0 when a prompt has no
    eos).  ids int32 / int64 [B, N] on the GPU, z bf16 [B*N, C] contiguous.  The position is found on the device."""
    if not ids.is_cuda:
        raise ValueError("clip_pool_eos.ids: expected a GPU tensor (anyedit_amd has no CPU path)")
    if ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 2 or not ids.is_contiguous():
        raise TypeError(f"clip_pool_eos.ids: expected a contiguous int32 / int64 [B, N] tensor, got {ids.dtype} {tuple(ids.shape)}")
    _chk(z, BF16, "clip_pool_eos.z", 2)
    B, N = ids.shape
    C = z.shape[1]
    if z.shape[0] != B * N or not z.is_contiguous():
        raise ValueError(f"clip_pool_eos: z must be a contiguous [{B * N}, C] buffer")
    if out is None:
        out = torch.empty(B, C, dtype=BF16, device=z.device)
    _chk(out, BF16, "clip_pool_eos.out", 2)
    if tuple(out.shape) != (B, C) or not out.is_contiguous():
        raise ValueError(f"clip_pool_eos: out must be a contiguous [{B}, {C}] buffer")
    check(lib.ae_clip_pool_eos_bf16(_p(ids), 1 if ids.dtype == torch.int64 else 0, _p(z), _p(out), B, N, C, int(eos_token_id), _s()), "ae_clip_pool_eos_bf16")
    return out


# --------------------------------------------------------------------------- CLIP vision tower (csrc/clip_vision.hip)
_PX_DTYPES = {torch.float32: 0, BF16: 1, torch.uint8: 2}


def clip_patch_kpad(Cin, P):
    """Columns of a patch row: Cin * P * P rounded up to a multiple of 64 (P = 14: 588 -> 640)."""
    return (Cin * P * P + 63) // 64 * 64


def pack_patch_embedding(w):
    """CLIPVisionEmbeddings.patch_embedding.weight [C, Cin, P, P] -> bf16 [C, Kpad]: flattened, zero-padded to `clip_patch_kpad` columns
    (the weight image that goes with `clip_patch_rows`)."""
    C, Cin, P, P2 = w.shape
    if P != P2:
        raise ValueError(f"pack_patch_embedding: square patches only, got {P}x{P2}")
    out = torch.zeros(C, clip_patch_kpad(Cin, P), dtype=BF16, device=w.device)
    out[:, :Cin * P * P] = w.detach().reshape(C, -1).to(BF16)
    return out


def clip_patch_rows(x, P, rescale=1.0, mean=None, std=None, out=None):
    """im2col of the CLIP patch embedding with the image processor's rescale + normalise fused in: x [B, Cin, H, W] (fp32, bf16 or uint8,
    contiguous, H % P == W % P == 0) -> bf16 rows [B*(H/P)*(W/P), Kpad]; column c*P*P + ky*P + kx = (x * rescale - mean[c]) / std[c]
    (mean = std = None: x * rescale), pad columns written as zeros."""
    if not x.is_cuda:
        raise ValueError("clip_patch_rows.x: expected a GPU tensor (anyedit_amd has no CPU path)")
    if x.dtype not in _PX_DTYPES or x.dim() != 4 or not x.is_contiguous():
        raise TypeError(f"clip_patch_rows.x: expected a contiguous fp32 / bf16 / uint8 [B, Cin, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    B, Cin, H, W = x.shape
    if P <= 0 or H % P or W % P:
        raise ValueError(f"clip_patch_rows: image {H}x{W} is not a whole number of {P}x{P} patches")
    if (mean is None) != (std is None):
        raise ValueError("clip_patch_rows: mean and std go together")
    if mean is not None:
        _chk(mean, torch.float32, "clip_patch_rows.mean", 1)
        _chk(std, torch.float32, "clip_patch_rows.std", 1)
        if mean.numel() != Cin or std.numel() != Cin or not mean.is_contiguous() or not std.is_contiguous():
            raise ValueError(f"clip_patch_rows: mean and std need one value per channel ({Cin})")
    M, Kpad = B * (H // P) * (W // P), clip_patch_kpad(Cin, P)
    if out is None:
        out = torch.empty(M, Kpad, dtype=BF16, device=x.device)
    _chk(out, BF16, "clip_patch_rows.out", 2)
    if tuple(out.shape) != (M, Kpad) or not out.is_contiguous():
        raise ValueError(f"clip_patch_rows: out must be a contiguous [{M}, {Kpad}] buffer")
    check(lib.ae_clip_patch_rows_bf16(_p(x), _PX_DTYPES[x.dtype], _p(out), B, Cin, H, W, P, Kpad, float(rescale), _p(mean), _p(std), _s()),
          "ae_clip_patch_rows_bf16")
    return out


def clip_vision_embed_ln(patch, class_embedding, pos, gamma, beta, eps, B, out=None):
    """Token rows + pre_layrnorm of the CLIP vision tower in one launch: out[b, 0] = LN(class_embedding + pos[0]), out[b, 1 + i] =
    LN(patch[b*G + i] + pos[1 + i]) -> bf16 [B*(1+G), C].  patch: the fp32 [B*G, C] product of `gemm(rows, Wpatch, out_f32=True)`;
    class_embedding [C], pos [1+G, C], gamma / beta [C] fp32.  C % 8 == 0, C <= 2048."""
    _chk(patch, torch.float32, "clip_vision_embed_ln.patch", 2)
    _chk(class_embedding, torch.float32, "clip_vision_embed_ln.class_embedding", 1)
    _chk(pos, torch.float32, "clip_vision_embed_ln.pos", 2)
    _chk(gamma, torch.float32, "clip_vision_embed_ln.gamma", 1)
    _chk(beta, torch.float32, "clip_vision_embed_ln.beta", 1)
    M, C = patch.shape
    if B <= 0 or M % B:
        raise ValueError(f"clip_vision_embed_ln: {M} patch rows do not split into {B} samples")
    G = M // B
    if patch.stride(1) != 1 or tuple(pos.shape) != (G + 1, C) or not pos.is_contiguous() or class_embedding.numel() != C or gamma.numel() != C or beta.numel() != C:
        raise ValueError(f"clip_vision_embed_ln: need patch rows of unit inner stride, pos [{G + 1}, {C}] contiguous and class_embedding / gamma / beta of {C} values")
    if out is None:
        out = torch.empty(B * (G + 1), C, dtype=BF16, device=patch.device)
    _chk(out, BF16, "clip_vision_embed_ln.out", 2)
    if tuple(out.shape) != (B * (G + 1), C) or not out.is_contiguous():
        raise ValueError(f"clip_vision_embed_ln: out must be a contiguous [{B * (G + 1)}, {C}] buffer")
    check(lib.ae_clip_vision_embed_ln_bf16(_p(patch), patch.stride(0), _p(class_embedding), _p(pos), _p(gamma), _p(beta), _p(out), B, G, C, float(eps), _s()),
          "ae_clip_vision_embed_ln_bf16")
    return out


def clip_vision_pool_ln(x, N, gamma, beta, eps, out=None):
    """post_layernorm of the class rows only: x bf16 [B*N, C] contiguous -> LN(x[b*N]) as bf16 [B, C] (the other rows are not read)."""
    _chk(x, BF16, "clip_vision_pool_ln.x", 2)
    _chk(gamma, torch.float32, "clip_vision_pool_ln.gamma", 1)
    _chk(beta, torch.float32, "clip_vision_pool_ln.beta", 1)
    M, C = x.shape
    if N <= 0 or M % N or not x.is_contiguous() or gamma.numel() != C or beta.numel() != C:
        raise ValueError(f"clip_vision_pool_ln: x must be a contiguous [B*{N}, C] buffer with gamma / beta of C values, got {tuple(x.shape)}")
    B = M // N
    if out is None:
        out = torch.empty(B, C, dtype=BF16, device=x.device)
    _chk(out, BF16, "clip_vision_pool_ln.out", 2)
    if tuple(out.shape) != (B, C) or not out.is_contiguous():
        raise ValueError(f"clip_vision_pool_ln: out must be a contiguous [{B}, {C}] buffer")
    check(lib.ae_clip_vision_pool_ln_bf16(_p(x), N * C, _p(gamma), _p(beta), _p(out), B, C, float(eps), _s()), "ae_clip_vision_pool_ln_bf16")
    return out


# --------------------------------------------------------------------------- DINOv2 image encoder (csrc/dino_vision.hip)
def dino_embed(patch, patch_bias, cls_token, pos, B, out=None):
    """Token rows of DinoVisionTransformer (prepare_tokens_with_masks): out[b, 0] = cls_token + pos[0], out[b, 1 + i] = patch[b*G + i] +
    patch_bias + pos[1 + i] -> bf16 [B*(1+G), C], rounded once.  patch: the fp32 [B*G, C] product of `gemm(rows, Wpatch, out_f32=True)` (row
    stride free); patch_bias / cls_token [C], pos [1+G, C] fp32 (the table interpolated to this grid).  No LayerNorm.  C % 8 == 0."""
    _chk(patch, torch.float32, "dino_embed.patch", 2)
    _chk(patch_bias, torch.float32, "dino_embed.patch_bias", 1)
    _chk(cls_token, torch.float32, "dino_embed.cls_token", 1)
    _chk(pos, torch.float32, "dino_embed.pos", 2)
    M, C = patch.shape
    if B <= 0 or M % B:
        raise ValueError(f"dino_embed: {M} patch rows do not split into {B} samples")
    G = M // B
    if patch.stride(1) != 1 or tuple(pos.shape) != (G + 1, C) or not pos.is_contiguous() or cls_token.numel() != C or patch_bias.numel() != C:
        raise ValueError(f"dino_embed: need patch rows of unit inner stride, pos [{G + 1}, {C}] contiguous and cls_token / patch_bias of {C} values")
    if out is None:
        out = torch.empty(B * (G + 1), C, dtype=BF16, device=patch.device)
    _chk(out, BF16, "dino_embed.out", 2)
    if tuple(out.shape) != (B * (G + 1), C) or not out.is_contiguous():
        raise ValueError(f"dino_embed: out must be a contiguous [{B * (G + 1)}, {C}] buffer")
    check(lib.ae_dino_embed_bf16(_p(patch), patch.stride(0), _p(patch_bias), _p(cls_token), _p(pos), _p(out), B, G, C, _s()), "ae_dino_embed_bf16")
    return out


def swiglu(u, bias, out=None):
    """y[m, j] = silu(u[m, j] + bias[j]) * (u[m, Hd + j] + bias[Hd + j]) as bf16, u the fp32 [M, 2*Hd] product of `gemm(..., out_f32=True)` with
    SwiGLUFFN's w12 (row stride free): the pre-activation is never rounded.  out: [M, Hd] bf16 with unit inner stride; where its row stride
    is wider than Hd, the columns between Hd and the stride are written as zeros.  Hd % 8 == 0."""
    _chk(u, torch.float32, "swiglu.u", 2)
    _chk(bias, torch.float32, "swiglu.bias", 1)
    M, N2 = u.shape
    if N2 % 2 or u.stride(1) != 1 or bias.numel() != N2 or not bias.is_contiguous():
        raise ValueError("swiglu: u needs an even number of columns and unit inner stride, bias one value per column")
    Hd = N2 // 2
    if out is None:
        out = torch.empty(M, Hd, dtype=BF16, device=u.device)
    _chk(out, BF16, "swiglu.out", 2)
    if tuple(out.shape) != (M, Hd) or out.stride(1) != 1:
        raise ValueError(f"swiglu: out must be [{M}, {Hd}] with unit inner stride")
    check(lib.ae_swiglu_f32_bf16(_p(u), u.stride(0), _p(bias), _p(out), out.stride(0), M, Hd, _s()), "ae_swiglu_f32_bf16")
    return out


# --------------------------------------------------------------------------- GroundingDINO's Swin backbone (csrc/swin.hip)
SWIN_HEAD_DIM = 32
SWIN_MAX_WINDOW = 16
SWIN_MERGE_CMAX = 1024


def swin_window_attention(qkv, qkv_bias, bias, B, H, W, heads, window, shift, scale, out=None):
    """Shifted-window attention of one Swin block on rows in IMAGE order: qkv bf16 [B*H*W, 3C] (unit inner stride, row stride free: the packed
    q | k | v of `gemm(norm1(x), Wqkv, bqkv)`), qkv_bias fp32 [3C] (what a pad token's key and value are), bias fp32 [heads, N, N] contiguous
    (N = window^2: the gathered relative position bias) -> out bf16 [B*H*W, C].  Pad, cyclic shift, window partition, the -100 shift mask, window
    reverse, shift back and crop are the kernel's row addressing.  head_dim C / heads must be 32, window <= 16, 0 <= shift < window."""
    _chk(qkv, BF16, "swin_window_attention.qkv", 2)
    _chk(qkv_bias, torch.float32, "swin_window_attention.qkv_bias", 1)
    _chk(bias, torch.float32, "swin_window_attention.bias", 3)
    M, C3 = qkv.shape
    if C3 % 3 or qkv.stride(1) != 1:
        raise ValueError(f"swin_window_attention: qkv must be [rows, 3C] with unit inner stride, got {tuple(qkv.shape)}")
    C = C3 // 3
    if heads <= 0 or C % heads or C // heads != SWIN_HEAD_DIM:
        raise ValueError(f"swin_window_attention: head_dim {C}/{heads} must be {SWIN_HEAD_DIM} (the only one ae_swin_window_attn_bf16 is built for)")
    if not 1 <= window <= SWIN_MAX_WINDOW:
        raise ValueError(f"swin_window_attention: window size {window} must be in [1, {SWIN_MAX_WINDOW}]")
    if not 0 <= shift < window:
        raise ValueError(f"swin_window_attention: shift {shift} must be in [0, window size {window})")
    if B <= 0 or H <= 0 or W <= 0 or M != B * H * W:
        raise ValueError(f"swin_window_attention: {M} rows are not B*H*W = {B}*{H}*{W}")
    N = window * window
    if tuple(bias.shape) != (heads, N, N) or not bias.is_contiguous():
        raise ValueError(f"swin_window_attention: bias must be a contiguous [{heads}, {N}, {N}] tensor, got {tuple(bias.shape)}")
    if qkv_bias.numel() != C3 or not qkv_bias.is_contiguous():
        raise ValueError(f"swin_window_attention: qkv_bias must hold {C3} values")
    if out is None:
        out = torch.empty(M, C, dtype=BF16, device=qkv.device)
    _chk(out, BF16, "swin_window_attention.out", 2)
    if tuple(out.shape) != (M, C) or out.stride(1) != 1:
        raise ValueError(f"swin_window_attention: out must be [{M}, {C}] with unit inner stride")
    check(lib.ae_swin_window_attn_bf16(_p(qkv), qkv.stride(0), _p(qkv_bias), _p(bias), _p(out), out.stride(0), B, H, W, C, heads, window, shift, float(scale),
                                       _s()), "ae_swin_window_attn_bf16")
    return out


def swin_merge_layernorm(x, gamma, beta, B, H, W, eps=1e-5, out=None):
    """PatchMerging up to its norm: x bf16 [B*H*W, C] contiguous (rows of an H x W map) -> LayerNorm over 4C of cat(x(2i, 2j), x(2i+1, 2j),
    x(2i, 2j+1), x(2i+1, 2j+1)) as bf16 [B*ceil(H/2)*ceil(W/2), 4C]; positions outside an odd map are zeros that enter the statistics.
    gamma / beta fp32 [4C].  C % 8 == 0, C <= 1024."""
    _chk(x, BF16, "swin_merge_layernorm.x", 2)
    _chk(gamma, torch.float32, "swin_merge_layernorm.gamma", 1)
    _chk(beta, torch.float32, "swin_merge_layernorm.beta", 1)
    M, C = x.shape
    if B <= 0 or H <= 0 or W <= 0 or M != B * H * W or not x.is_contiguous():
        raise ValueError(f"swin_merge_layernorm: x must be a contiguous [B*H*W, C] = [{B}*{H}*{W}, C] buffer, got {tuple(x.shape)}")
    if C % 8 or C > SWIN_MERGE_CMAX:
        raise ValueError(f"swin_merge_layernorm: width {C} must be a multiple of 8 and at most {SWIN_MERGE_CMAX}")
    if gamma.numel() != 4 * C or beta.numel() != 4 * C or not gamma.is_contiguous() or not beta.is_contiguous():
        raise ValueError(f"swin_merge_layernorm: gamma and beta must hold 4C = {4 * C} values")
    M2 = B * ((H + 1) // 2) * ((W + 1) // 2)
    if out is None:
        out = torch.empty(M2, 4 * C, dtype=BF16, device=x.device)
    _chk(out, BF16, "swin_merge_layernorm.out", 2)
    if tuple(out.shape) != (M2, 4 * C) or not out.is_contiguous():
        raise ValueError(f"swin_merge_layernorm: out must be a contiguous [{M2}, {4 * C}] buffer")
    check(lib.ae_swin_merge_ln_bf16(_p(x), _p(gamma), _p(beta), _p(out), B, H, W, C, float(eps), _s()), "ae_swin_merge_ln_bf16")
    return out


# --------------------------------------------------------------------------- GroundingDINO's feature enhancer (csrc/gdino_encoder.hip)
BIATTN_HEAD_DIM = 256
BIATTN_MAX_TEXT = 256
MASKED_SHORT_MAX_N = 256
_BIATTN_WS = {}


def bi_attention_split_rows(Nv):
    """Image tokens per partial of the text direction of `bi_attention` (ae_biattn_split_rows): it is merged from ceil(Nv / rows) partials."""
    return lib.ae_biattn_split_rows(int(Nv))


def _rows3(t, name, B, N, C):
    _chk(t, BF16, name, 3)
    if tuple(t.shape) != (B, N, C) or t.stride(2) != 1 or (B > 1 and t.stride(0) != N * t.stride(1)):
        raise ValueError(f"{name}: expected [{B}, {N}, {C}] rows with unit inner stride and one row stride over all samples, got shape {tuple(t.shape)} "
                         f"strides {tuple(t.stride())}")
    return t.stride(1)


def bi_attention(q, k, val_v, val_l, heads, scale, mask_v=None, mask_l=None, out_v=None, out_l=None):
    """The two attentions of BiMultiHeadAttention (fuse_modules.py:174-225) over ONE logit matrix scale q k^T, head_dim 256:
        out_v [B, Nv, heads*256] = softmax over text keys (mask_l removed) of the logits, times val_l
        out_l [B, Nt, heads*256] = softmax over image keys (mask_v removed) of the transposed logits, times val_v
    q / val_v: bf16 [B, Nv, heads*256], k / val_l: bf16 [B, Nt, heads*256] (unit inner stride, any row stride).  mask_v [B, Nv] / mask_l [B, Nt]:
    bool or uint8, True = a PADDED token (the reference's sense), removed as a key; rows of padded queries are computed like any others.
    CONTRACT, not checked (it would be a host synchronisation): every sample has at least one unmasked text token and one unmasked image token.
    The global-maximum subtraction and the +-50000 clamps of the reference are left out (include/anyedit_hip.h).  Nt in [1, 256], Nv >= 1.  No
    buffer of size ~ Nv*Nt exists; the workspace (ae_biattn_workspace_bytes) is grow-only per (device, stream), so a warmed-up call allocates
    nothing besides outputs the caller did not pass."""
    _chk(q, BF16, "bi_attention.q", 3)
    _chk(k, BF16, "bi_attention.k", 3)
    B, Nv, C = q.shape
    Nt = k.shape[1]
    if heads <= 0 or C % heads or C // heads != BIATTN_HEAD_DIM:
        raise ValueError(f"bi_attention: head_dim {C}/{heads} must be {BIATTN_HEAD_DIM} (the only one ae_biattn_bf16 is built for)")
    if not 1 <= Nt <= BIATTN_MAX_TEXT:
        raise ValueError(f"bi_attention: {Nt} text tokens; ae_biattn_bf16 takes between 1 and {BIATTN_MAX_TEXT}")
    if Nv < 1:
        raise ValueError("bi_attention: no image tokens")
    ldq, ldk = _rows3(q, "bi_attention.q", B, Nv, C), _rows3(k, "bi_attention.k", B, Nt, C)
    ldvv, ldvl = _rows3(val_v, "bi_attention.val_v", B, Nv, C), _rows3(val_l, "bi_attention.val_l", B, Nt, C)
    if out_v is None:
        out_v = torch.empty(B, Nv, C, dtype=BF16, device=q.device)
    if out_l is None:
        out_l = torch.empty(B, Nt, C, dtype=BF16, device=q.device)
    ldov, ldol = _rows3(out_v, "bi_attention.out_v", B, Nv, C), _rows3(out_l, "bi_attention.out_l", B, Nt, C)
    masks = []
    for m, n, name in ((mask_v, Nv, "mask_v"), (mask_l, Nt, "mask_l")):
        if m is not None:
            if m.dtype == torch.bool:
                m = m.view(torch.uint8)
            _chk(m, torch.uint8, "bi_attention." + name, 2)
            if tuple(m.shape) != (B, n) or not m.is_contiguous():
                raise ValueError(f"bi_attention: {name} must be a contiguous [{B}, {n}] bool / uint8 tensor, got {tuple(m.shape)}")
        masks.append(m)
    need = lib.ae_biattn_workspace_bytes(B, heads, Nv, Nt, BIATTN_HEAD_DIM)
    if need <= 0:
        raise ValueError(f"bi_attention: unsupported sizes B={B} heads={heads} Nv={Nv} Nt={Nt}")
    key = (q.device, torch.cuda.current_stream(q.device).cuda_stream)
    ws = _BIATTN_WS.get(key)
    if ws is None or ws.numel() < need:  # grow-only scratch per (device, stream): the call owns it until the next call on that stream
        ws = _BIATTN_WS[key] = torch.empty(need, dtype=torch.uint8, device=q.device)
    check(lib.ae_biattn_bf16(_p(q), ldq, _p(k), ldk, _p(val_v), ldvv, _p(val_l), ldvl, _p(masks[0]), _p(masks[1]), _p(out_v), ldov, _p(out_l), ldol,
                             B, heads, Nv, Nt, BIATTN_HEAD_DIM, float(scale), _p(ws), ws.numel(), _s()), "ae_biattn_bf16")
    return out_v, out_l


def scale_residual(u, res, gamma=None, bias=None, out=None):
    """out = res + gamma * (u + bias) as bf16, one rounding: u fp32 [M, N] (unit inner stride), res bf16 [M, N], gamma / bias fp32 [N] or None
    (1 / 0).  BiAttentionBlock's layer-scaled residual and the residual behind the fp32 deformable attention."""
    _chk(u, torch.float32, "scale_residual.u", 2)
    _chk(res, BF16, "scale_residual.res", 2)
    M, N = u.shape
    if tuple(res.shape) != (M, N) or u.stride(1) != 1 or res.stride(1) != 1:
        raise ValueError(f"scale_residual: u and res must both be [{M}, {N}] with unit inner stride")
    for t, n in ((gamma, "gamma"), (bias, "bias")):
        if t is not None:
            _chk(t, torch.float32, "scale_residual." + n, 1)
            if t.numel() != N or not t.is_contiguous():
                raise ValueError(f"scale_residual: {n} must hold {N} values")
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=u.device)
    _chk(out, BF16, "scale_residual.out", 2)
    if tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise ValueError(f"scale_residual: out must be [{M}, {N}] with unit inner stride")
    check(lib.ae_scale_residual_f32_bf16(_p(u), u.stride(0), _p(bias), _p(gamma), _p(res), res.stride(0), _p(out), out.stride(0), M, N, _s()),
          "ae_scale_residual_f32_bf16")
    return out


def attention_masked_short(q, k, v, mask, B, H, N, D, scale, q_strides, k_strides, v_strides, out=None):
    """Self-attention over at most 256 tokens with a full boolean mask (GroundingDINO's text layers): q/k/v bf16 tensors addressed through
    (batch, head, row) element strides as in `attention_causal_short`; mask uint8 (or bool) [B*H, N, N] contiguous, slice b*H + h, True = the key
    is ALLOWED for that query row; out [B, N, H*D] bf16.  CONTRACT: every row allows at least one key.  N in [1, 256], D in {32, 64}."""
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    return _attention_short("attention_masked_short", lib.ae_attn_masked_short_bf16, q, k, v, (mask, torch.uint8, "mask", (B * H, N, N)), B, H, N, D, scale,
                            q_strides, k_strides, v_strides, out, MASKED_SHORT_MAX_N, (32, 64))


# --------------------------------------------------------------------------- GroundingDINO text side (csrc/gdino_text.hip)
TEXT_SPANS_MAX_N = 256
BERT_EMBED_MAX_C = 2048


def _ids2(t, name):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a GPU tensor (anyedit_amd has no CPU path)")
    if t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous int32 / int64 [B, N] tensor, got {t.dtype} {tuple(t.shape)}")


def gdino_text_spans(ids, special_ids, spans=None, position_ids=None, dense_mask=None, want_mask=False):
    """bertwarper.py:180-273 in one launch, no host synchronisation: ids int32 / int64 [B, N] (N <= 256), `special_ids` up to 8 python ints ->
    (spans int32 [B, N, 2] = the key range [lo, hi) of every query, position_ids int64 [B, N], dense bool [B, N, N] mask or None).  The dense
    mask is written when `want_mask` or a `dense_mask` buffer (bool / uint8) is given.  CONTRACT: column 0 of every row is a special token."""
    _ids2(ids, "gdino_text_spans.ids")
    B, N = ids.shape
    if not 1 <= N <= TEXT_SPANS_MAX_N:
        raise ValueError(f"gdino_text_spans: {N} tokens; ae_gdino_text_spans takes between 1 and {TEXT_SPANS_MAX_N}")
    sp = [int(s) for s in special_ids]
    if len(sp) > 8:
        raise ValueError(f"gdino_text_spans: {len(sp)} special ids (at most 8)")
    dev = ids.device
    if spans is None:
        spans = torch.empty(B, N, 2, dtype=torch.int32, device=dev)
    if position_ids is None:
        position_ids = torch.empty(B, N, dtype=torch.int64, device=dev)
    if dense_mask is None and want_mask:
        dense_mask = torch.empty(B, N, N, dtype=torch.bool, device=dev)
    _chk(spans, torch.int32, "gdino_text_spans.spans", 3)
    _chk(position_ids, torch.int64, "gdino_text_spans.position_ids", 2)
    if tuple(spans.shape) != (B, N, 2) or not spans.is_contiguous() or tuple(position_ids.shape) != (B, N) or not position_ids.is_contiguous():
        raise ValueError(f"gdino_text_spans: spans must be a contiguous [{B}, {N}, 2] and position_ids a contiguous [{B}, {N}] buffer")
    if dense_mask is not None:
        if not dense_mask.is_cuda or dense_mask.dtype not in (torch.bool, torch.uint8) or tuple(dense_mask.shape) != (B, N, N) or not dense_mask.is_contiguous():
            raise ValueError(f"gdino_text_spans: dense_mask must be a contiguous bool / uint8 [{B}, {N}, {N}] GPU buffer")
    check(lib.ae_gdino_text_spans(_p(ids), 1 if ids.dtype == torch.int64 else 0, B, N, len(sp), *(sp + [0] * (8 - len(sp))), _p(spans), _p(position_ids),
                                  _p(dense_mask), _s()), "ae_gdino_text_spans")
    return spans, position_ids, dense_mask


def bert_embed_ln(ids, word, position, token_type, gamma, beta, eps, position_ids=None, type_ids=None, out=None):
    """BertEmbeddings in one launch: LayerNorm(word[ids] + position[position_ids] + token_type[type_ids]) -> bf16 rows [B*N, C]; the sum is never
    stored.  ids (and position_ids / type_ids; None = n / row 0) int64 [B, N]; tables bf16, gamma / beta fp32.
    Indices are NOT read back: one outside its table is clamped into it by the kernel."""
    _ids2(ids, "bert_embed_ln.ids")
    B, N = ids.shape
    for t, n in ((ids, "ids"), (position_ids, "position_ids"), (type_ids, "type_ids")):
        if t is not None:
            _ids2(t, "bert_embed_ln." + n)
            if t.dtype != torch.int64 or tuple(t.shape) != (B, N):
                raise TypeError(f"bert_embed_ln.{n}: expected int64 [{B}, {N}], got {t.dtype} {tuple(t.shape)}")
    for t, n in ((word, "word"), (position, "position"), (token_type, "token_type")):
        _chk(t, BF16, "bert_embed_ln." + n, 2)
    _chk(gamma, torch.float32, "bert_embed_ln.gamma", 1)
    _chk(beta, torch.float32, "bert_embed_ln.beta", 1)
    C = word.shape[1]
    if C % 8 or C > BERT_EMBED_MAX_C:
        raise ValueError(f"bert_embed_ln: width {C} must be a multiple of 8 and at most {BERT_EMBED_MAX_C}")
    if position.shape[1] != C or token_type.shape[1] != C or gamma.numel() != C or beta.numel() != C or \
            not (word.is_contiguous() and position.is_contiguous() and token_type.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()):
        raise ValueError(f"bert_embed_ln: the three tables must be contiguous [rows, {C}] and gamma / beta hold {C} values")
    if position_ids is None and N > position.shape[0]:
        raise ValueError(f"bert_embed_ln: {N} tokens, the position table has {position.shape[0]} rows")
    if out is None:
        out = torch.empty(B * N, C, dtype=BF16, device=ids.device)
    _chk(out, BF16, "bert_embed_ln.out", 2)
    if tuple(out.shape) != (B * N, C) or not out.is_contiguous():
        raise ValueError(f"bert_embed_ln: out must be a contiguous [{B * N}, {C}] buffer")
    check(lib.ae_bert_embed_ln_bf16(_p(ids), _p(position_ids), _p(type_ids), _p(word), _p(position), _p(token_type),
                                    _p(gamma), _p(beta), _p(out), B, N, C, word.shape[0], position.shape[0], token_type.shape[0], float(eps), _s()),
          "ae_bert_embed_ln_bf16")
    return out


def attention_span_short(q, k, v, spans, B, H, N, D, scale, q_strides, k_strides, v_strides, out=None):
    """Self-attention over at most 256 tokens under a block-diagonal mask (BERT under GroundingDINO's sub-sentence masks): q/k/v bf16 tensors
    addressed through (batch, head, row) element strides as in `attention_masked_short`; spans int32 [B, N, 2] contiguous, shared by all heads:
    query n attends keys [lo, hi); out [B, N, H*D] bf16.  CONTRACT: 0 <= lo < hi <= N.  N in [1, 256], D == 64."""
    return _attention_short("attention_span_short", lib.ae_attn_span_short_bf16, q, k, v, (spans, torch.int32, "spans", (B, N, 2)), B, H, N, D, scale,
                            q_strides, k_strides, v_strides, out, TEXT_SPANS_MAX_N, (64,))


# --------------------------------------------------------------------------- GroundingDINO query selection / decoder (csrc/gdino_decoder.hip)
CONTRASTIVE_MAX_TEXT = 256
CONTRASTIVE_MAX_C = 256
TOPK_MAX_K = 1024


def _mask2(m, name, B, n):
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    _chk(m, torch.uint8, name, 2)
    if tuple(m.shape) != (B, n) or not m.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous [{B}, {n}] bool / uint8 tensor, got {tuple(m.shape)}")
    return m


def contrastive(x, y, token_mask=None, max_text_len=None, want_logits=True, want_rowmax=False, logits=None, rowmax=None):
    """ContrastiveEmbed.forward (utils.py:233-268) and / or its row maximum (transformer.py:295).  x bf16 [B, N, C] (unit inner stride, one row
    stride over all samples), y bf16 [B, T, C] contiguous, token_mask bool / uint8 [B, T], True = a USED token (the reference's text_token_mask).
    Returns (logits, rowmax), either None when not asked for: logits fp32 [B, N, max_text_len] with -inf at unused tokens and at columns
    T .. max_text_len-1, rowmax fp32 [B, N] (-inf when a sample has no used token).  With want_logits=False no B*N*T buffer exists.
    C % 32 == 0, C <= 256, 1 <= T <= max_text_len <= 256."""
    _chk(x, BF16, "contrastive.x", 3)
    _chk(y, BF16, "contrastive.y", 3)
    B, N, C = x.shape
    T = y.shape[1]
    max_text_len = T if max_text_len is None else int(max_text_len)
    if C % 32 or not 32 <= C <= CONTRASTIVE_MAX_C:
        raise ValueError(f"contrastive: C={C} must be a multiple of 32, at most {CONTRASTIVE_MAX_C}")
    if not 1 <= T <= max_text_len <= CONTRASTIVE_MAX_TEXT:
        raise ValueError(f"contrastive: need 1 <= T={T} <= max_text_len={max_text_len} <= {CONTRASTIVE_MAX_TEXT}")
    if N < 1:
        raise ValueError("contrastive: no rows")
    if tuple(y.shape) != (B, T, C) or not y.is_contiguous():
        raise ValueError(f"contrastive: y must be a contiguous [{B}, {T}, {C}] tensor, got {tuple(y.shape)}")
    ldx = _rows3(x, "contrastive.x", B, N, C)
    if token_mask is not None:
        token_mask = _mask2(token_mask, "contrastive.token_mask", B, T)
    want_logits = want_logits or logits is not None
    want_rowmax = want_rowmax or rowmax is not None
    if not (want_logits or want_rowmax):
        raise ValueError("contrastive: neither logits nor rowmax is asked for")
    ldl = 0
    if want_logits:
        if logits is None:
            logits = torch.empty(B, N, max_text_len, dtype=torch.float32, device=x.device)
        _chk(logits, torch.float32, "contrastive.logits", 3)
        if tuple(logits.shape) != (B, N, max_text_len) or logits.stride(2) != 1 or (B > 1 and logits.stride(0) != N * logits.stride(1)):
            raise ValueError(f"contrastive: logits must be [{B}, {N}, {max_text_len}] rows with unit inner stride and one row stride")
        ldl = logits.stride(1)
    if want_rowmax:
        if rowmax is None:
            rowmax = torch.empty(B, N, dtype=torch.float32, device=x.device)
        _chk(rowmax, torch.float32, "contrastive.rowmax", 2)
        if tuple(rowmax.shape) != (B, N) or not rowmax.is_contiguous():
            raise ValueError(f"contrastive: rowmax must be a contiguous [{B}, {N}] tensor")
    check(lib.ae_contrastive_bf16(_p(x), ldx, _p(y), _p(token_mask), _p(logits), ldl, _p(rowmax), B, N, T, C, max_text_len, _s()), "ae_contrastive_bf16")
    return logits, rowmax


def topk_rows_max_n():
    """Largest row length `topk_rows` takes (ae_topk_rows_max_n)."""
    return lib.ae_topk_rows_max_n()


def topk_rows(scores, k, out=None):
    """int32 [B, k]: the first k indices of torch.sort(scores, dim=1, descending=True, stable=True) — descending value, equal values by ascending
    index, -0.0 == +0.0, -inf an ordinary value, NaN of either sign above +inf.  scores fp32 [B, N] (unit inner stride).  torch.topk promises no
    order among ties; query selection meets ties on every masked image row.  1 <= k <= min(N, 1024), N <= topk_rows_max_n()."""
    _chk(scores, torch.float32, "topk_rows.scores", 2)
    B, N = scores.shape
    k = int(k)
    if B < 1 or N < 1 or scores.stride(1) != 1:
        raise ValueError(f"topk_rows: scores must be a non-empty [B, N] tensor with unit inner stride, got {tuple(scores.shape)}")
    if not 1 <= k <= min(N, TOPK_MAX_K):
        raise ValueError(f"topk_rows: k={k} must be in [1, min(N={N}, {TOPK_MAX_K})]")
    if N > topk_rows_max_n():
        raise ValueError(f"topk_rows: N={N} is above the largest supported row length {topk_rows_max_n()}")
    if out is None:
        out = torch.empty(B, k, dtype=torch.int32, device=scores.device)
    _chk(out, torch.int32, "topk_rows.out", 2)
    if tuple(out.shape) != (B, k) or not out.is_contiguous():
        raise ValueError(f"topk_rows: out must be a contiguous int32 [{B}, {k}] tensor")
    check(lib.ae_topk_rows_f32(_p(scores), scores.stride(0) if B > 1 else N, _p(out), B, N, k, _s()), "ae_topk_rows_f32")
    return out


def gdino_proposals(padding_mask, spatial_shapes, proposals=None, keep=None):
    """gen_encoder_output_proposals (utils.py:56-116, learnedwh=None) in one launch.  padding_mask bool / uint8 [B, N], True = padding;
    spatial_shapes: a HOST sequence of (H, W) per level with sum H*W == N (at most 8 levels).  Returns (proposals fp32 [B, N, 4] un-sigmoided,
    +inf on padded rows and rows outside 0.01 < p < 0.99; keep uint8 [B, N], 1 where the row's memory is kept)."""
    shapes = [(int(h), int(w)) for h, w in spatial_shapes]
    L = len(shapes)
    if padding_mask.dim() != 2:
        raise ValueError(f"gdino_proposals: padding_mask must be [B, N], got {tuple(padding_mask.shape)}")
    B, N = padding_mask.shape
    padding_mask = _mask2(padding_mask, "gdino_proposals.padding_mask", B, N)
    if not 1 <= L <= 8 or any(h < 1 or w < 1 for h, w in shapes) or sum(h * w for h, w in shapes) != N:
        raise ValueError(f"gdino_proposals: {L} levels {shapes} do not tile N={N} tokens (1 to 8 levels, each at least 1x1)")
    starts, cur = [], 0
    for h, w in shapes:
        starts.append(cur)
        cur += h * w
    if proposals is None:
        proposals = torch.empty(B, N, 4, dtype=torch.float32, device=padding_mask.device)
    if keep is None:
        keep = torch.empty(B, N, dtype=torch.uint8, device=padding_mask.device)
    _chk(proposals, torch.float32, "gdino_proposals.proposals", 3)
    _chk(keep, torch.uint8, "gdino_proposals.keep", 2)
    if tuple(proposals.shape) != (B, N, 4) or not proposals.is_contiguous() or tuple(keep.shape) != (B, N) or not keep.is_contiguous():
        raise ValueError(f"gdino_proposals: proposals must be contiguous [{B}, {N}, 4], keep contiguous [{B}, {N}]")
    c_shapes = (ctypes.c_int * (2 * L))(*[v for hw in shapes for v in hw])
    c_starts = (ctypes.c_int * L)(*starts)
    check(lib.ae_gdino_proposals_f32(_p(padding_mask), c_shapes, c_starts, L, _p(proposals), _p(keep), B, N, _s()), "ae_gdino_proposals_f32")
    return proposals, keep


def gdino_query_sine(reference_points, valid_ratios, ref_input=None, embed=None):
    """reference_points fp32 [B, nq, 4] (sigmoid boxes), valid_ratios fp32 [B, L, 2] -> (reference_points_input fp32 [B, nq, L, 4]
    (transformer.py:667-671), gen_sineembed_for_position of its level-0 slice as bf16 rows [B*nq, 512] in (y, x, w, h) order (utils.py:204-230))."""
    _chk(reference_points, torch.float32, "gdino_query_sine.reference_points", 3)
    _chk(valid_ratios, torch.float32, "gdino_query_sine.valid_ratios", 3)
    B, nq, four = reference_points.shape
    L = valid_ratios.shape[1]
    if four != 4 or B < 1 or nq < 1 or not reference_points.is_contiguous():
        raise ValueError(f"gdino_query_sine: reference_points must be a contiguous non-empty [B, nq, 4] tensor, got {tuple(reference_points.shape)}")
    if tuple(valid_ratios.shape) != (B, L, 2) or L < 1 or L > 64 or not valid_ratios.is_contiguous():
        raise ValueError(f"gdino_query_sine: valid_ratios must be a contiguous [{B}, L, 2] tensor with 1 <= L <= 64, got {tuple(valid_ratios.shape)}")
    if ref_input is None:
        ref_input = torch.empty(B, nq, L, 4, dtype=torch.float32, device=reference_points.device)
    if embed is None:
        embed = torch.empty(B * nq, 512, dtype=BF16, device=reference_points.device)
    _chk(ref_input, torch.float32, "gdino_query_sine.ref_input", 4)
    _chk(embed, BF16, "gdino_query_sine.embed", 2)
    if tuple(ref_input.shape) != (B, nq, L, 4) or not ref_input.is_contiguous() or tuple(embed.shape) != (B * nq, 512) or embed.stride(1) != 1:
        raise ValueError(f"gdino_query_sine: ref_input must be contiguous [{B}, {nq}, {L}, 4], embed [{B * nq}, 512] rows with unit inner stride")
    check(lib.ae_gdino_query_sine(_p(reference_points), _p(valid_ratios), _p(ref_input), _p(embed), embed.stride(0), B, nq, L, _s()), "ae_gdino_query_sine")
    return ref_input, embed


def gdino_box_refine(h, w3, b3, ref, ref_is_logit=False, want_unsigmoid=False, boxes=None, unsigmoid=None):
    """The last layer of a box MLP plus the anchor update (transformer.py:721-724, groundingdino.py:322-324): h fp32 [M, 256] (unit inner stride),
    w3 fp32 [4, 256], b3 fp32 [4], ref fp32 [M, 4] -> boxes = sigmoid(u), u = h w3^T + b3 + inverse_sigmoid(ref) (eps 1e-3), all fp32.
    ref_is_logit: ref is already un-sigmoided (it may be +inf: the box is then 1.0) and is added as it is (transformer.py:296-306).
    Returns boxes, or (boxes, u) with want_unsigmoid."""
    _chk(h, torch.float32, "gdino_box_refine.h", 2)
    _chk(w3, torch.float32, "gdino_box_refine.w3", 2)
    _chk(b3, torch.float32, "gdino_box_refine.b3", 1)
    _chk(ref, torch.float32, "gdino_box_refine.ref", 2)
    M = h.shape[0]
    if M < 1 or h.shape[1] != 256 or h.stride(1) != 1:
        raise ValueError(f"gdino_box_refine: h must be a non-empty [M, 256] tensor with unit inner stride, got {tuple(h.shape)}")
    if tuple(w3.shape) != (4, 256) or not w3.is_contiguous() or b3.numel() != 4 or not b3.is_contiguous():
        raise ValueError("gdino_box_refine: w3 must be contiguous [4, 256] and b3 hold 4 values")
    if tuple(ref.shape) != (M, 4) or not ref.is_contiguous():
        raise ValueError(f"gdino_box_refine: ref must be a contiguous [{M}, 4] tensor, got {tuple(ref.shape)}")
    if boxes is None:
        boxes = torch.empty(M, 4, dtype=torch.float32, device=h.device)
    want_unsigmoid = want_unsigmoid or unsigmoid is not None
    if want_unsigmoid and unsigmoid is None:
        unsigmoid = torch.empty(M, 4, dtype=torch.float32, device=h.device)
    for t, n in ((boxes, "boxes"), (unsigmoid, "unsigmoid")):
        if t is not None:
            _chk(t, torch.float32, "gdino_box_refine." + n, 2)
            if tuple(t.shape) != (M, 4) or not t.is_contiguous():
                raise ValueError(f"gdino_box_refine: {n} must be a contiguous [{M}, 4] tensor")
    check(lib.ae_gdino_box_refine_f32(_p(h), h.stride(0), _p(w3), _p(b3), _p(ref), _p(boxes), _p(unsigmoid), M, 1 if ref_is_logit else 0, _s()),
          "ae_gdino_box_refine_f32")
    return (boxes, unsigmoid) if want_unsigmoid else boxes


def _levels(spatial_shapes, what):
    shapes = [(int(h), int(w)) for h, w in spatial_shapes]
    if not 1 <= len(shapes) <= 8 or any(h < 1 or w < 1 for h, w in shapes):
        raise ValueError(f"{what}: {len(shapes)} levels {shapes} (1 to 8 levels, each at least 1x1)")
    starts, cur = [], 0
    for h, w in shapes:
        starts.append(cur)
        cur += h * w
    return shapes, starts, cur


def gdino_level_geometry(mask, spatial_shapes, B, temperatureH=20.0, temperatureW=20.0, level_embed=None, device=None, mask_flatten=None,
                         pos_flatten=None, valid_ratios=None):
    """Every level's padding mask, sine position embedding and valid ratios in one launch (backbone.py:113 and groundingdino.py:306's nearest
    resize of the image mask, position_encoding.py:98-131 with normalize=True, transformer.py's `+ level_embed[lvl]` and flatten / cat,
    Transformer.get_valid_ratio).  mask: bool / uint8 [B, H, W], True = padding, or None (nothing padded; pass `device`); spatial_shapes: a HOST
    sequence of (h, w) per level; level_embed fp32 [L, 256] or None.  Returns (mask_flatten bool [B, N], pos_flatten bf16 [B, N, 256],
    valid_ratios fp32 [B, L, 2]) with N = sum h w."""
    shapes, starts, N = _levels(spatial_shapes, "gdino_level_geometry")
    L = len(shapes)
    if mask is not None:
        if mask.dim() != 3 or mask.shape[0] != B or not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"gdino_level_geometry: mask must be a GPU bool / uint8 [{B}, H, W] tensor, got {mask.dtype} {tuple(mask.shape)}")
        mask = _tmp(mask.contiguous())
        H, W, device = mask.shape[1], mask.shape[2], mask.device
    else:
        if device is None:
            raise ValueError("gdino_level_geometry: pass device= when mask is None")
        H, W = shapes[0]
    if level_embed is not None:
        _chk(level_embed, torch.float32, "gdino_level_geometry.level_embed", 2)
        if tuple(level_embed.shape) != (L, 256) or not level_embed.is_contiguous():
            raise ValueError(f"gdino_level_geometry: level_embed must be contiguous [{L}, 256], got {tuple(level_embed.shape)}")
    if mask_flatten is None:
        mask_flatten = torch.empty(B, N, dtype=torch.bool, device=device)
    if pos_flatten is None:
        pos_flatten = torch.empty(B, N, 256, dtype=BF16, device=device)
    if valid_ratios is None:
        valid_ratios = torch.empty(B, L, 2, dtype=torch.float32, device=device)
    for t, dt, shp, n in ((mask_flatten, torch.bool, (B, N), "mask_flatten"), (pos_flatten, BF16, (B, N, 256), "pos_flatten"),
                          (valid_ratios, torch.float32, (B, L, 2), "valid_ratios")):
        _chk(t, dt, "gdino_level_geometry." + n)
        if tuple(t.shape) != shp or not t.is_contiguous():
            raise ValueError(f"gdino_level_geometry: {n} must be contiguous {list(shp)}, got {tuple(t.shape)}")
    c_shapes = (ctypes.c_int * (2 * L))(*[v for hw in shapes for v in hw])
    c_starts = (ctypes.c_int * L)(*starts)
    check(lib.ae_gdino_level_geometry(_p(mask), B, H, W, c_shapes, c_starts, L, float(temperatureH), float(temperatureW), _p(level_embed), _p(mask_flatten),
                                      _p(pos_flatten), _p(valid_ratios), N, _s()), "ae_gdino_level_geometry")
    return mask_flatten, pos_flatten, valid_ratios


NECK_GN_C = 256


def gdino_neck_groupnorm_workspace(B, hw, device):
    return torch.empty(max(1, lib.ae_gdino_neck_groupnorm_workspace_floats(B, hw)), dtype=torch.float32, device=device)


def gdino_neck_groupnorm(x, gamma, beta, B, hw, eps=1e-5, out=None, row_offset=0, workspace=None):
    """GroupNorm(32, 256) of input_proj (groundingdino.py:127-138) on the fp32 projection.  x fp32 [B*hw, 256] (unit inner stride: ops.gemm /
    ops.conv3x3 with out_f32=True); gamma / beta fp32 [256]; out bf16 [B, N, 256] contiguous with N >= row_offset + hw: sample b's rows go to
    out[b, row_offset : row_offset + hw] (a level's slice of src_flatten); None = a fresh [B, hw, 256].  Returns out."""
    _chk(x, torch.float32, "gdino_neck_groupnorm.x", 2)
    _chk(gamma, torch.float32, "gdino_neck_groupnorm.gamma", 1)
    _chk(beta, torch.float32, "gdino_neck_groupnorm.beta", 1)
    if B < 1 or hw < 1 or tuple(x.shape) != (B * hw, NECK_GN_C) or x.stride(1) != 1:
        raise ValueError(f"gdino_neck_groupnorm: x must be [{B} * {hw}, {NECK_GN_C}] with unit inner stride, got {tuple(x.shape)}")
    if gamma.numel() != NECK_GN_C or beta.numel() != NECK_GN_C or not gamma.is_contiguous() or not beta.is_contiguous():
        raise ValueError(f"gdino_neck_groupnorm: gamma and beta must hold {NECK_GN_C} contiguous values")
    if out is None:
        out = torch.empty(B, hw, NECK_GN_C, dtype=BF16, device=x.device)
    _chk(out, BF16, "gdino_neck_groupnorm.out", 3)
    if out.shape[0] != B or out.shape[2] != NECK_GN_C or not out.is_contiguous() or row_offset < 0 or row_offset + hw > out.shape[1]:
        raise ValueError(f"gdino_neck_groupnorm: out must be contiguous [{B}, N, {NECK_GN_C}] with N >= {row_offset} + {hw}, got {tuple(out.shape)}")
    need = lib.ae_gdino_neck_groupnorm_workspace_floats(B, hw)
    if workspace is None:
        workspace = _tmp(gdino_neck_groupnorm_workspace(B, hw, x.device))
    _chk(workspace, torch.float32, "gdino_neck_groupnorm.workspace", 1)
    if workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError(f"gdino_neck_groupnorm: workspace holds {workspace.numel()} floats, {need} are needed")
    check(lib.ae_gdino_neck_groupnorm(_p(x), x.stride(0), _p(gamma), _p(beta), float(eps), _p(out), out.stride(0), row_offset, B, hw, _p(workspace), _s()),
          "ae_gdino_neck_groupnorm")
    return out


GROUND_MAX_QUERIES = 1024
GROUND_MAX_TEXT = 256


def gdino_ground(pred_logits, pred_boxes, box_threshold, text_threshold, out=None):
    """get_grounding_output's filter (AnyEdit_Collection/adaptive_editing_pipelines/tools/tool.py:125-133) on the GPU.  pred_logits fp32
    [B, nq, T] (T a multiple of 32, at most 256; -inf on unused columns), pred_boxes fp32 [B, nq, 4].  Returns (count int32 [B], indices int32
    [B, nq], scores fp32 [B, nq], boxes fp32 [B, nq, 4], token_bits int32 [B, nq, T // 32]): the first count[b] rows hold the queries with
    max_t sigmoid(logit) > box_threshold in ascending query order; bit t % 32 of word t // 32 says sigmoid(logit_t) > text_threshold.  `out`: the
    same tuple from an earlier call of the same shape, to be overwritten."""
    _chk(pred_logits, torch.float32, "gdino_ground.pred_logits", 3)
    _chk(pred_boxes, torch.float32, "gdino_ground.pred_boxes", 3)
    B, nq, T = pred_logits.shape
    if B < 1 or not 1 <= nq <= GROUND_MAX_QUERIES or T % 32 or not 32 <= T <= GROUND_MAX_TEXT or not pred_logits.is_contiguous():
        raise ValueError(f"gdino_ground: pred_logits must be contiguous [B, nq <= {GROUND_MAX_QUERIES}, T] with T a multiple of 32 up to {GROUND_MAX_TEXT}, "
                         f"got {tuple(pred_logits.shape)}")
    if tuple(pred_boxes.shape) != (B, nq, 4) or not pred_boxes.is_contiguous():
        raise ValueError(f"gdino_ground: pred_boxes must be contiguous [{B}, {nq}, 4], got {tuple(pred_boxes.shape)}")
    dev = pred_logits.device
    shapes = ((B,), (B, nq), (B, nq), (B, nq, 4), (B, nq, T // 32))
    dts = (torch.int32, torch.int32, torch.float32, torch.float32, torch.int32)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dts))
    for t, s, d in zip(out, shapes, dts):
        _chk(t, d, "gdino_ground.out")
        if tuple(t.shape) != s or not t.is_contiguous():
            raise ValueError(f"gdino_ground: an output must be contiguous {list(s)}, got {tuple(t.shape)}")
    count, idx, scores, boxes, bits = out
    check(lib.ae_gdino_ground(_p(pred_logits), _p(pred_boxes), float(box_threshold), float(text_threshold), _p(count), _p(idx), _p(scores), _p(boxes), _p(bits),
                              B, nq, T, _s()), "ae_gdino_ground")
    return out


# --------------------------------------------------------------------------- HED edge detector (csrc/hed.hip)
HED_STEM_CMAX = 512
HED_LEVELS = 5
HED_MIN_SIDE = 1 << (HED_LEVELS - 1)      # below it the fifth side map is empty
HED_MAX_SIDE = 16384


def _out_buf(out, dtype, shape, name, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    return _target(out, dtype, shape, name)


def hed_stem(x, norm, w, bias, out=None):
    """relu(conv3x3(x - norm, w) + bias) -> bf16 channels-last rows [B*H*W, C1], in one launch.  x: a uint8 image batch [B, H, W, 3] or fp32
    [B, 3, H, W] (any strides: the kernel addresses it by element strides); norm fp32 of 3 values, w fp32 [C1, 3, 3, 3], bias fp32 [C1], C1 % 8
    == 0 and at most 512.  The zero padding applies to x - norm.  Returns (rows, B, H, W)."""
    if not x.is_cuda:
        raise ValueError("hed_stem.x: expected a GPU tensor (anyedit_amd has no CPU path)")
    if x.dim() != 4:
        raise ValueError(f"hed_stem: x must be uint8 [B, H, W, 3] or fp32 [B, 3, H, W], got shape {tuple(x.shape)}")
    if x.dtype == torch.uint8:
        B, H, W, C = x.shape
        sb, sh, sw, sc = x.stride()
    elif x.dtype == torch.float32:
        B, C, H, W = x.shape
        sb, sc, sh, sw = x.stride()
    else:
        raise TypeError(f"hed_stem.x: expected torch.uint8 [B, H, W, 3] or torch.float32 [B, 3, H, W], got {x.dtype}")
    if C != 3 or B < 1 or H < 1 or W < 1:
        raise ValueError(f"hed_stem: x must be uint8 [B, H, W, 3] or fp32 [B, 3, H, W], got shape {tuple(x.shape)}")
    norm = _dense(norm, torch.float32, "hed_stem.norm")
    w = _dense(w, torch.float32, "hed_stem.w", 4)
    bias = _dense(bias, torch.float32, "hed_stem.bias", 1)
    C1 = w.shape[0]
    if tuple(w.shape) != (C1, 3, 3, 3) or norm.numel() != 3 or bias.numel() != C1:
        raise ValueError(f"hed_stem: need w [C1, 3, 3, 3], norm of 3 values and bias [C1], got {tuple(w.shape)}, {tuple(norm.shape)}, {tuple(bias.shape)}")
    out = _out_buf(out, BF16, (B * H * W, C1), "hed_stem.out", x.device)
    check(lib.ae_hed_stem_bf16(_p(x), 1 if x.dtype == torch.float32 else 0, sb, sc, sh, sw, _p(norm), _p(w), _p(bias), _p(out), B, H, W, C1, _s()),
          "ae_hed_stem_bf16")
    return out, B, H, W


def relu_(x):
    """ReLU in place on a contiguous bf16 tensor; returns it."""
    _chk(x, BF16, "relu_.x")
    if not x.is_contiguous() or x.numel() == 0:
        raise ValueError("relu_: x must be a contiguous, non-empty tensor (the kernel writes it in place)")
    check(lib.ae_relu_bf16(_p(x), x.numel(), _s()), "ae_relu_bf16")
    return x


def hed_tail(y, wp, bp, B, H, W, pool=True, proj=None, pooled=None):
    """The end of a HED block on its last convolution's output y BEFORE the ReLU (bf16 rows [B*H*W, C], C % 8 == 0), in one pass:
    proj fp32 [B, H, W] = sum_c relu(y)[c] * wp[c] + bp (fp32 weights wp [C], bp of one value, fp32 accumulation) and, with `pool`, pooled bf16
    rows [B*(H//2)*(W//2), C] = max_pool2d(relu(y), 2, 2).  Returns (proj, pooled or None)."""
    _chk(y, BF16, "hed_tail.y", 2)
    C = y.shape[1]
    if y.shape[0] != B * H * W or not y.is_contiguous() or B < 1 or H < 1 or W < 1:
        raise ValueError(f"hed_tail: y must be contiguous [B*H*W, C] = [{B * H * W}, C], got {tuple(y.shape)}")
    wp = _dense(wp, torch.float32, "hed_tail.wp").reshape(-1)
    bp = _dense(bp, torch.float32, "hed_tail.bp").reshape(-1)
    if wp.numel() != C or bp.numel() != 1:
        raise ValueError(f"hed_tail: need {C} projection weights and one bias, got {wp.numel()} and {bp.numel()}")
    proj = _out_buf(proj, torch.float32, (B, H, W), "hed_tail.proj", y.device)
    if pool:
        if H < 2 or W < 2:
            raise ValueError(f"hed_tail: a {H} x {W} map has no 2x2 window to pool")
        pooled = _out_buf(pooled, BF16, (B * (H // 2) * (W // 2), C), "hed_tail.pooled", y.device)
    elif pooled is not None:
        raise ValueError("hed_tail: a pooled buffer was given with pool=False")
    check(lib.ae_hed_tail_bf16(_p(y), _p(wp), _p(bp), _p(proj), _p(pooled), B, H, W, C, _s()), "ae_hed_tail_bf16")
    return proj, pooled


def hed_fuse(sides, invert=True, out=None, logits=None, want_logits=False):
    """HEDdetector's arithmetic after the network: the five fp32 side maps [B, H >> k, W >> k] (or [B, 1, h, w]) resized to H x W (bilinear,
    half-pixel centres, edge clamp), averaged, sigmoid, * 255, clip, truncated to uint8 [B, H, W]; `invert`: 255 - v.  With `want_logits` (or a
    `logits` buffer) the fp32 mean before the sigmoid is written too.  Returns the uint8 map, or (map, logits)."""
    if len(sides) != HED_LEVELS:
        raise ValueError(f"hed_fuse: expected {HED_LEVELS} side maps, got {len(sides)}")
    s0 = sides[0]
    _chk(s0, torch.float32, "hed_fuse.sides[0]")
    if s0.dim() == 4 and s0.shape[1] == 1:
        sides = [s.squeeze(1) if s.dim() == 4 else s for s in sides]
        s0 = sides[0]
    if s0.dim() != 3:
        raise ValueError(f"hed_fuse: side maps must be [B, h, w] or [B, 1, h, w], got {tuple(s0.shape)}")
    B, H, W = s0.shape
    if not (HED_MIN_SIDE <= H <= HED_MAX_SIDE and HED_MIN_SIDE <= W <= HED_MAX_SIDE):
        raise ValueError(f"hed_fuse: sides of {HED_MIN_SIDE} .. {HED_MAX_SIDE} pixels are covered, got {H} x {W}")
    dense = []
    for k, s in enumerate(sides):
        _chk(s, torch.float32, f"hed_fuse.sides[{k}]", 3)
        if tuple(s.shape) != (B, H >> k, W >> k):
            raise ValueError(f"hed_fuse: side map {k} must be [{B}, {H >> k}, {W >> k}], got {tuple(s.shape)}")
        dense.append(_tmp(s.contiguous()))
    out = _out_buf(out, torch.uint8, (B, H, W), "hed_fuse.out", s0.device)
    if want_logits or logits is not None:
        logits = _out_buf(logits, torch.float32, (B, H, W), "hed_fuse.logits", s0.device)
    check(lib.ae_hed_fuse(*[_p(s) for s in dense], _p(out), _p(logits), B, H, W, 1 if invert else 0, _s()), "ae_hed_fuse")
    return out if logits is None else (out, logits)


# --------------------------------------------------------------------------- Depth Anything V2's DPT head (csrc/dpt.hip)
DPT_MAX_SIDE = 16384
DPT_STRIDES = (1, 2, 4)


def _rows(t, name, rows, C=None):
    """a contiguous bf16 row buffer [rows, C] with C % 8 == 0"""
    _chk(t, BF16, name, 2)
    if t.shape[0] != rows or not t.is_contiguous() or (C is not None and t.shape[1] != C):
        raise ValueError(f"{name}: expected contiguous rows [{rows}, {'C' if C is None else C}], got {tuple(t.shape)} strides {t.stride()}")
    if t.shape[1] % 8 or t.shape[1] < 8:
        raise ValueError(f"{name}: {t.shape[1]} channels: the kernel takes 8 channels (16 bytes) per lane, C must be a multiple of 8")
    return t


def _sides(what, *sides):
    if any(s < 1 or s > DPT_MAX_SIDE for s in sides):
        raise ValueError(f"{what}: sides of 1 .. {DPT_MAX_SIDE} are covered, got {sides}")


def dpt_reassemble(prod, bias, B, gh, gw, k, out=None):
    """The data movement of DPTHead's `projects[i]` + `resize_layers[i]` after their products.  prod: fp32 [B * (1 + gh gw), k k oc] (row stride free,
    a multiple of 4), one row per token with each image's class row first, columns (ky k + kx) oc + c; bias fp32 [oc].  Returns bf16 rows
    [B * (gh k) * (gw k), oc] = bf16(prod + bias) at pixel (gy k + ky, gx k + kx); the class rows are skipped.  k in {1, 2, 4}."""
    _chk(prod, torch.float32, "dpt_reassemble.prod", 2)
    if k not in DPT_STRIDES:
        raise ValueError(f"dpt_reassemble: k={k} is not covered (the head's resize layers have strides {DPT_STRIDES})")
    if B < 1 or gh < 1 or gw < 1:
        raise ValueError(f"dpt_reassemble: bad sizes B={B} grid {gh}x{gw}")
    _sides("dpt_reassemble", gh * k, gw * k)
    bias = _dense(bias, torch.float32, "dpt_reassemble.bias", 1)
    oc = bias.numel()
    if oc % 8 or oc < 8:
        raise ValueError(f"dpt_reassemble: oc={oc} must be a multiple of 8 (16 bytes per lane)")
    if tuple(prod.shape) != (B * (1 + gh * gw), k * k * oc) or prod.stride(1) != 1 or prod.stride(0) % 4 or prod.stride(0) < k * k * oc:
        raise ValueError(f"dpt_reassemble: prod must be [B * (1 + gh gw), k k oc] = [{B * (1 + gh * gw)}, {k * k * oc}] with unit inner stride and a row "
                         f"stride that is a multiple of 4, got {tuple(prod.shape)} strides {prod.stride()}")
    out = _out_buf(out, BF16, (B * gh * k * gw * k, oc), "dpt_reassemble.out", prod.device)
    check(lib.ae_dpt_reassemble_bf16(_p(prod), prod.stride(0), _p(bias), _p(out), B, gh, gw, k, oc, _s()), "ae_dpt_reassemble_bf16")
    return out


def dpt_resize(x, B, h, w, H, W, addend=None, out=None, relu_out=None, want_relu=False):
    """F.interpolate(mode="bilinear", align_corners=True) on channels-last bf16 rows: x [B*h*w, C] -> [B*H*W, C], any two sizes (a side of 1
    included), + `addend` ([B*H*W, C] bf16) in fp32 before the single rounding.  With `want_relu` (or a `relu_out` buffer) relu(result) is written
    too.  Returns the rows, or (rows, relu rows)."""
    if B < 1:
        raise ValueError(f"dpt_resize: bad batch {B}")
    _sides("dpt_resize", h, w, H, W)
    _rows(x, "dpt_resize.x", B * h * w)
    C = x.shape[1]
    if addend is not None:
        _rows(addend, "dpt_resize.addend", B * H * W, C)
    out = _out_buf(out, BF16, (B * H * W, C), "dpt_resize.out", x.device)
    if want_relu or relu_out is not None:
        relu_out = _out_buf(relu_out, BF16, (B * H * W, C), "dpt_resize.relu_out", x.device)
    check(lib.ae_dpt_resize_bf16(_p(x), _p(addend), _p(out), _p(relu_out), B, h, w, H, W, C, _s()), "ae_dpt_resize_bf16")
    return out if relu_out is None else (out, relu_out)


def dpt_relu(x, out=None):
    """relu(x) out of place on contiguous bf16 rows [rows, C], C % 8 == 0 (`relu_` is the in-place form)."""
    _chk(x, BF16, "dpt_relu.x", 2)
    _rows(x, "dpt_relu.x", x.shape[0])
    out = _out_buf(out, BF16, tuple(x.shape), "dpt_relu.out", x.device)
    if out.data_ptr() == x.data_ptr():
        raise ValueError("dpt_relu: out must not be x (relu_ is the in-place form)")
    check(lib.ae_dpt_relu_bf16(_p(x), _p(out), x.numel(), _s()), "ae_dpt_relu_bf16")
    return out


def dpt_tail(y, wp, bp, B, H, W, out=None):
    """The end of the head on y, the rows [B*H*W, C] of `output_conv2[0]` BEFORE its ReLU: fp32 depth [B, H, W] = relu(sum_c relu(y)[c] wp[c] + bp),
    fp32 weights wp [C] and bp of one value, fp32 accumulation.  (`DepthAnythingV2.forward`'s own F.relu of this is a no-op.)"""
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"dpt_tail: bad sizes B={B} {H}x{W}")
    _rows(y, "dpt_tail.y", B * H * W)
    C = y.shape[1]
    wp = _dense(wp, torch.float32, "dpt_tail.wp").reshape(-1)
    bp = _dense(bp, torch.float32, "dpt_tail.bp").reshape(-1)
    if wp.numel() != C or bp.numel() != 1:
        raise ValueError(f"dpt_tail: need {C} projection weights and one bias, got {wp.numel()} and {bp.numel()}")
    out = _out_buf(out, torch.float32, (B, H, W), "dpt_tail.out", y.device)
    check(lib.ae_dpt_tail_bf16(_p(y), _p(wp), _p(bp), _p(out), B, H, W, C, _s()), "ae_dpt_tail_bf16")
    return out


def depth_resize_minmax(depth, H, W, out=None, minmax=None):
    """fp32 depth [B, h, w] -> ([B, H, W], minmax [B, 2]): F.interpolate(mode="bilinear", align_corners=True) and each image's (minimum, maximum)
    of the values written, bit-equal to out.amin((1, 2)) / out.amax((1, 2)) whatever the order the blocks finish in."""
    depth = _dense(depth, torch.float32, "depth_resize_minmax.depth", 3)
    B, h, w = depth.shape
    if B < 1 or B > 65535:
        raise ValueError(f"depth_resize_minmax: batches of 1 .. 65535 are covered, got {B}")
    _sides("depth_resize_minmax", h, w, H, W)
    out = _out_buf(out, torch.float32, (B, H, W), "depth_resize_minmax.out", depth.device)
    minmax = _out_buf(minmax, torch.float32, (B, 2), "depth_resize_minmax.minmax", depth.device)
    if out.data_ptr() == depth.data_ptr():
        raise ValueError("depth_resize_minmax: out must not be the input")
    check(lib.ae_depth_resize_minmax_f32(_p(depth), _p(out), _p(minmax), B, h, w, H, W, _s()), "ae_depth_resize_minmax_f32")
    return out, minmax


def depth_colorize(depth, minmax, table, out=None):
    """img2depth's colour image: uint8 [B, H, W, 3] = table[uint8((d - min) / (max - min) * 255.0)], fp32 with IEEE division and truncation; depth
    fp32 [B, H, W], minmax fp32 [B, 2] on the device (read by the kernel: no host synchronisation), table uint8 [256, 3].  An image whose max equals
    its min (0 / 0 in the reference) gets table[0] everywhere."""
    depth = _dense(depth, torch.float32, "depth_colorize.depth", 3)
    B, H, W = depth.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"depth_colorize: bad sizes {tuple(depth.shape)}")
    minmax = _dense(minmax, torch.float32, "depth_colorize.minmax", 2)
    table = _dense(table, torch.uint8, "depth_colorize.table", 2)
    if tuple(minmax.shape) != (B, 2) or tuple(table.shape) != (256, 3):
        raise ValueError(f"depth_colorize: need minmax [{B}, 2] and a [256, 3] table, got {tuple(minmax.shape)} and {tuple(table.shape)}")
    out = _out_buf(out, torch.uint8, (B, H, W, 3), "depth_colorize.out", depth.device)
    check(lib.ae_depth_colorize_u8(_p(_tmp(depth)), _p(_tmp(minmax)), _p(_tmp(table)), _p(out), B, H, W, _s()), "ae_depth_colorize_u8")
    return out


# --------------------------------------------------------------------------- UniFormer backbone (csrc/uniformer.hip)
DWCONV_KERNELS = (3, 5)
LN_NCHW_CMAX = 1024


def pack_dwconv(w):
    """Depthwise nn.Conv2d weight [C, 1, k, k] -> fp32 [k*k, C], tap-major (row ky * k + kx): the weight image of `dwconv`.  Stays fp32."""
    C, one, k, k2 = w.shape
    if one != 1 or k != k2 or k not in DWCONV_KERNELS:
        raise ValueError(f"pack_dwconv: expected a depthwise [C, 1, k, k] weight with k in {DWCONV_KERNELS}, got {tuple(w.shape)}")
    return w.detach().float().reshape(C, k * k).t().contiguous()


def pack_patch2(w):
    """nn.Conv2d(Cin, Cout, kernel_size=2, stride=2) weight [Cout, Cin, 2, 2] -> bf16 [Cout, 4*Cin], column (2 ky + kx) * Cin + cin: the weight
    image that goes with the rows of `patch2_rows`."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (2, 2):
        raise ValueError(f"pack_patch2: expected a [Cout, Cin, 2, 2] weight, got {tuple(w.shape)}")
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(BF16).contiguous()


def dwconv(x, w, bias, B, H, W, residual=None, out=None):
    """Depthwise k x k convolution (stride 1, zero padding k // 2) on bf16 rows [B*H*W, C]: out = bf16(residual + bias + sum_taps w x), fp32
    accumulation.  w: `pack_dwconv` image, fp32 [k*k, C] with k in {3, 5}; bias fp32 [C]; residual: optional rows, x itself allowed.  Out of
    place: `out` must not be x."""
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"dwconv: bad sizes B={B} {H}x{W}")
    _rows(x, "dwconv.x", B * H * W)
    C = x.shape[1]
    _chk(w, torch.float32, "dwconv.w", 2)
    _chk(bias, torch.float32, "dwconv.bias", 1)
    k = {kk * kk: kk for kk in DWCONV_KERNELS}.get(w.shape[0])
    if k is None or w.shape[1] != C or not w.is_contiguous() or bias.numel() != C or not bias.is_contiguous():
        raise ValueError(f"dwconv: need a contiguous [k*k, {C}] weight image with k in {DWCONV_KERNELS} and a bias of {C}, got {tuple(w.shape)} and "
                         f"{tuple(bias.shape)}")
    if residual is not None:
        _rows(residual, "dwconv.residual", B * H * W, C)
    out = _out_buf(out, BF16, (B * H * W, C), "dwconv.out", x.device)
    check(lib.ae_dwconv_rows_bf16(_p(x), _p(w), _p(bias), _p(residual), _p(out), B, H, W, C, k, _s()), "ae_dwconv_rows_bf16")
    return out


def patch2_rows(x, B, H, W, out=None):
    """bf16 rows [B*H*W, C] -> [B*(H//2)*(W//2), 4*C], column (2 ky + kx) * C + c (the order of `pack_patch2`); an odd last row or column is
    dropped.  Returns (rows, H // 2, W // 2)."""
    if B < 1 or H < 2 or W < 2:
        raise ValueError(f"patch2_rows: a {H} x {W} map (batch {B}) is below the 2x2 patch")
    _rows(x, "patch2_rows.x", B * H * W)
    C = x.shape[1]
    out = _out_buf(out, BF16, (B * (H // 2) * (W // 2), 4 * C), "patch2_rows.out", x.device)
    check(lib.ae_patch2_rows_bf16(_p(x), _p(out), B, H, W, C, _s()), "ae_patch2_rows_bf16")
    return out, H // 2, W // 2


def layernorm_rows_nchw(x, gamma, beta, eps, B, H, W, out=None, rows=None, want_rows=False):
    """LayerNorm over C of bf16 rows [B*H*W, C], written as fp32 [B, C, H, W] in one launch; with `want_rows` (or a `rows` buffer) the normalised
    bf16 rows too.  Returns the map, or (map, rows)."""
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"layernorm_rows_nchw: bad sizes B={B} {H}x{W}")
    _rows(x, "layernorm_rows_nchw.x", B * H * W)
    C = x.shape[1]
    if C > LN_NCHW_CMAX:
        raise ValueError(f"layernorm_rows_nchw: rows of up to {LN_NCHW_CMAX} channels are covered, got {C}")
    _chk(gamma, torch.float32, "layernorm_rows_nchw.gamma", 1)
    _chk(beta, torch.float32, "layernorm_rows_nchw.beta", 1)
    if gamma.numel() != C or beta.numel() != C or not gamma.is_contiguous() or not beta.is_contiguous():
        raise ValueError(f"layernorm_rows_nchw: gamma and beta need {C} contiguous values")
    out = _out_buf(out, torch.float32, (B, C, H, W), "layernorm_rows_nchw.out", x.device)
    if want_rows or rows is not None:
        rows = _out_buf(rows, BF16, (B * H * W, C), "layernorm_rows_nchw.rows", x.device)
    check(lib.ae_layernorm_rows_nchw(_p(x), _p(gamma), _p(beta), float(eps), _p(out), _p(rows), B, H, W, C, _s()), "ae_layernorm_rows_nchw")
    return out if rows is None else (out, rows)


# --------------------------------------------------------------------------- UPerNet head and the segment map (csrc/upernet.hip)
UP_MAX_SIDE = 16384
PPM_MAX_SCALES, PPM_MAX_SCALE = 4, 8
RESIZE_CONCAT_MAX_SOURCES = 5
SEG_MAX_CLASSES = 256


def fold_bn_after_conv(weight, gamma, beta, mean, var, eps):
    """A BatchNorm in eval mode directly behind a bias-free convolution (mmcv's ConvModule): s (W x - mean) + beta = (W s) x + (beta - mean s) with
    s = gamma / sqrt(var + eps) per OUTPUT channel.  weight [Cout, Cin, k, k]; returns (weight scaled per output channel, bias [Cout]) in the dtype
    of the arguments: the modules fold in fp32, before the rounding to bf16."""
    s = gamma / torch.sqrt(var + eps)
    return weight * s.view(-1, *([1] * (weight.dim() - 1))), beta - mean * s


def _up_sides(what, *sides):
    if any(s < 1 or s > UP_MAX_SIDE for s in sides):
        raise ValueError(f"{what}: sides of 1 .. {UP_MAX_SIDE} are covered, got {sides}")


def ppm_pool(x, B, H, W, scales, out=None):
    """Every nn.AdaptiveAvgPool2d(s) of a pooling pyramid in one launch: bf16 rows [B*H*W, C] -> [B * sum(s*s), C]; within an image scale k's s*s
    bins follow scale k-1's, row-major.  Up to 4 scales of 1 .. 8 each; fp32 mean, one rounding."""
    scales = tuple(int(s) for s in scales)
    if not 1 <= len(scales) <= PPM_MAX_SCALES or any(s < 1 or s > PPM_MAX_SCALE for s in scales):
        raise ValueError(f"ppm_pool: 1 .. {PPM_MAX_SCALES} pool scales of 1 .. {PPM_MAX_SCALE} each are covered, got {scales}")
    if B < 1:
        raise ValueError(f"ppm_pool: bad batch {B}")
    _up_sides("ppm_pool", H, W)
    _rows(x, "ppm_pool.x", B * H * W)
    C = x.shape[1]
    out = _out_buf(out, BF16, (B * sum(s * s for s in scales), C), "ppm_pool.out", x.device)
    arr = (ctypes.c_int * len(scales))(*scales)
    check(lib.ae_ppm_pool_rows_bf16(_p(x), _p(out), B, H, W, C, arr, len(scales), _s()), "ae_ppm_pool_rows_bf16")
    return out


def resize_concat(sources, dst, B, H, W, addend=None):
    """F.interpolate(mode="bilinear", align_corners=False) of up to five sources into column slices of `dst`, bf16 rows [B*H*W, ld] (contiguous), in
    one launch.  sources: [(rows, h, w, col, relu), ...] with rows bf16 [B*h*w, C] or [B, h*w, C] (unit inner stride, any row and image stride that is a
    multiple of 8: a slice of a wider buffer), col
    the first destination column of the slice, relu: max(tap, 0) as the taps are read.  A source of the destination's size is copied bit for bit.
    addend: optional bf16 rows [B*H*W, C], with a single source only, added in fp32 before the rounding; it may be the destination's slice itself.
    The columns of dst outside the slices are not touched.  Returns dst."""
    n = len(sources)
    if not 1 <= n <= RESIZE_CONCAT_MAX_SOURCES:
        raise ValueError(f"resize_concat: 1 .. {RESIZE_CONCAT_MAX_SOURCES} sources per launch, got {n}")
    if B < 1:
        raise ValueError(f"resize_concat: bad batch {B}")
    _up_sides("resize_concat", H, W)
    _chk(dst, BF16, "resize_concat.dst", 2)
    if dst.shape[0] != B * H * W or not dst.is_contiguous() or dst.shape[1] % 8:
        raise ValueError(f"resize_concat: dst must be contiguous rows [{B * H * W}, ld] with ld a multiple of 8, got {tuple(dst.shape)} strides {dst.stride()}")
    ld = dst.shape[1]
    spans, views = [], []
    for i, (rows, h, w, col, relu) in enumerate(sources):
        _up_sides(f"resize_concat.sources[{i}]", h, w)
        _chk(rows, BF16, f"resize_concat.sources[{i}]")
        if rows.dim() == 2 and rows.shape[0] == B * h * w:
            rows = rows.as_strided((B, h * w, rows.shape[1]), (h * w * rows.stride(0), rows.stride(0), 1), rows.storage_offset())
        if rows.dim() == 3 and (rows.shape[2] % 8 or rows.shape[2] < 8):
            raise ValueError(f"resize_concat.sources[{i}]: {rows.shape[2]} channels: the kernel takes 8 channels (16 bytes) per lane, C must be a multiple of 8")
        if rows.dim() != 3 or tuple(rows.shape[:2]) != (B, h * w) or rows.stride(2) != 1 or rows.stride(1) % 8 or rows.stride(0) % 8:
            raise ValueError(f"resize_concat.sources[{i}]: expected rows [{B * h * w}, C] or [{B}, {h * w}, C] with unit inner stride and row / image strides "
                             f"that are multiples of 8, got {tuple(rows.shape)} strides {rows.stride()}")
        C = rows.shape[2]
        views.append(rows)
        if col < 0 or col % 8 or col + C > ld:
            raise ValueError(f"resize_concat.sources[{i}]: columns {col} .. {col + C} do not fit the destination's {ld} (slices start at multiples of 8)")
        if any(col < c1 and c0 < col + C for c0, c1 in spans):
            raise ValueError(f"resize_concat.sources[{i}]: its slice overlaps an earlier one")
        spans.append((col, col + C))
    ld_add = 0
    if addend is not None:
        if n != 1:
            raise ValueError("resize_concat: the addend goes with a single source")
        _chk(addend, BF16, "resize_concat.addend", 2)
        C = views[0].shape[2]
        if tuple(addend.shape) != (B * H * W, C) or addend.stride(1) != 1 or addend.stride(0) % 8:
            raise ValueError(f"resize_concat.addend: expected rows [{B * H * W}, {C}], got {tuple(addend.shape)} strides {addend.stride()}")
        ld_add = addend.stride(0)
    vp, ci, cl = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_long * n
    check(lib.ae_resize_concat_rows_bf16(vp(*[_p(v) for v in views]), ci(*[s[1] for s in sources]), ci(*[s[2] for s in sources]),
                                         ci(*[v.shape[2] for v in views]), cl(*[v.stride(1) for v in views]), cl(*[v.stride(0) for v in views]), ci(*[s[3] for s in sources]),
                                         ci(*[1 if s[4] else 0 for s in sources]), n, _p(addend), ld_add, _p(dst), ld, B, H, W, _s()),
          "ae_resize_concat_rows_bf16")
    return dst


def seg_argmax(logits, ncls, B, h, w, mid, out_size=None, palette=None, labels=None, colours=None):
    """The end of EncoderDecoder.simple_test in one launch: logits fp32 rows [B*h*w, ld] (classes in the first `ncls` <= 256 columns, ld % 4 == 0; the
    columns from ncls on are never read) resized (h, w) -> mid = (Hm, Wm) -> out_size = (Ho, Wo) (bilinear, align_corners=False, the second stage
    skipped when the sizes agree), then the argmax over the classes, the lowest index among equals.  Returns uint8 labels [B, Ho, Wo], or with a
    uint8 palette [ncls, 3] (labels, colours uint8 [B, Ho, Wo, 3] = palette[label])."""
    _chk(logits, torch.float32, "seg_argmax.logits", 2)
    Hm, Wm = mid
    Ho, Wo = out_size if out_size is not None else mid
    if B < 1:
        raise ValueError(f"seg_argmax: bad batch {B}")
    _up_sides("seg_argmax", h, w, Hm, Wm, Ho, Wo)
    if not 1 <= ncls <= SEG_MAX_CLASSES:
        raise ValueError(f"seg_argmax: {ncls} classes: 1 .. {SEG_MAX_CLASSES} are covered (a uint8 label)")
    if logits.shape[0] != B * h * w or logits.shape[1] < ncls or logits.stride(1) != 1 or logits.stride(0) % 4 or logits.stride(0) < logits.shape[1]:
        raise ValueError(f"seg_argmax: logits must be rows [{B * h * w}, >= {ncls}] with unit inner stride and a row stride that is a multiple of 4, got "
                         f"{tuple(logits.shape)} strides {logits.stride()}")
    if palette is not None:
        palette = _dense(palette, torch.uint8, "seg_argmax.palette", 2)
        if tuple(palette.shape) != (ncls, 3):
            raise ValueError(f"seg_argmax: the palette must be uint8 [{ncls}, 3], got {tuple(palette.shape)}")
        colours = _out_buf(colours, torch.uint8, (B, Ho, Wo, 3), "seg_argmax.colours", logits.device)
    elif colours is not None:
        raise ValueError("seg_argmax: a colour buffer was given without a palette")
    labels = _out_buf(labels, torch.uint8, (B, Ho, Wo), "seg_argmax.labels", logits.device)
    check(lib.ae_seg_argmax_u8(_p(logits), logits.stride(0), ncls, _p(_tmp(palette)), _p(labels), _p(colours), B, h, w, Hm, Wm, Ho, Wo, _s()), "ae_seg_argmax_u8")
    return labels if palette is None else (labels, colours)


# --------------------------------------------------------------------------- MasaCtrl mutual self-attention (csrc/masactrl.hip)
MUTUAL_HEAD_DIMS = (40, 64, 80, 160)
MUTUAL_MAX_BATCH = 64
TOKEN_MAP_MAX_KEYS, TOKEN_MAP_MAX_DIM = 128, 160
MASACTRL_MAX_PAIRS = 8
CLS_ANY = 255


def _cls_buf(t, name, B, N):
    _chk(t, torch.uint8, name, 2)
    if tuple(t.shape) != (B, N) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous uint8 [{B}, {N}] tensor, got {tuple(t.shape)}")


def attention_mutual(q, k, v, B, H, N, D, scale, q_strides, k_strides, v_strides, src, qcls=None, kcls=None, kcnt=None, out=None, o_strides=None):
    """Self-attention in which sample b's queries read the keys / values of sample src[b] (ae_attn_mutual_bf16).  q/k/v: bf16 tensors addressed via
    (batch, head, row) element strides, as `attention` takes them; src: B host ints.  qcls uint8 [B, N] (255 = any key), kcls uint8 [B, N] and kcnt int32
    [B, 2] (class counts per sample, as `masactrl_classes` writes them; both indexed by src[b]): key j is allowed for query (b, i) iff qcls is None, or
    qcls[b, i] == 255, or kcls[src[b], j] == qcls[b, i]; a query whose class has no key in its source gets the mean of V.  out: [B, N, H*D] bf16."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, BF16, "attention_mutual." + n)
    if D not in MUTUAL_HEAD_DIMS:
        raise ValueError(f"attention_mutual: head dims {MUTUAL_HEAD_DIMS} are covered, got {D}")
    src = tuple(int(s) for s in src)
    if len(src) != B or B < 1 or B > MUTUAL_MAX_BATCH or any(s < 0 or s >= B for s in src):
        raise ValueError(f"attention_mutual: src needs {B} sample indices in [0, {B}) (B <= {MUTUAL_MAX_BATCH}), got {src}")
    if N < 1 or H < 1:
        raise ValueError(f"attention_mutual: bad sizes H={H} N={N}")
    if qcls is not None:
        if kcls is None or kcnt is None:
            raise ValueError("attention_mutual: qcls needs kcls and kcnt")
        _cls_buf(qcls, "attention_mutual.qcls", B, N)
        _cls_buf(kcls, "attention_mutual.kcls", B, N)
        _chk(kcnt, torch.int32, "attention_mutual.kcnt", 2)
        if tuple(kcnt.shape) != (B, 2) or not kcnt.is_contiguous():
            raise ValueError(f"attention_mutual.kcnt: expected a contiguous int32 [{B}, 2] tensor, got {tuple(kcnt.shape)}")
    elif kcls is not None or kcnt is not None:
        raise ValueError("attention_mutual: kcls / kcnt without qcls")
    if out is None:
        out = torch.empty(B, N, H * D, dtype=BF16, device=q.device)
    else:
        _chk(out, BF16, "attention_mutual.out")
    if o_strides is None:
        o_strides = (N * H * D, D, H * D)
    arr = (ctypes.c_int * B)(*src)
    check(lib.ae_attn_mutual_bf16(_p(q), _p(k), _p(v), _p(out), B, H, N, D, *q_strides, *k_strides, *v_strides, *o_strides, float(scale), arr,
                                  _p(qcls), _p(kcls), _p(kcnt), _s()), "ae_attn_mutual_bf16")
    return out


def token_set_words(tokens):
    """(low, high) uint64 words of a token set: bit j set iff token j (0 .. 127) is in `tokens`"""
    lo = hi = 0
    for t in tokens:
        t = int(t)
        if not 0 <= t < TOKEN_MAP_MAX_KEYS:
            raise ValueError(f"token set: token indices 0 .. {TOKEN_MAP_MAX_KEYS - 1} are covered, got {t}")
        if t < 64:
            lo |= 1 << t
        else:
            hi |= 1 << (t - 64)
    return lo, hi


def attention_token_map(q, k, B, H, N, Nk, D, scale, q_strides, k_strides, token_sets, out=None, accumulate=False):
    """Head-averaged softmax probabilities of a short-key attention summed over a per-sample token set (ae_attn_token_map_bf16):
    out[b, i] (+)= 1/H sum_h sum_{j in token_sets[b]} softmax_j(scale q[b,h,i] . k[b,h,j]); out fp32 [B, N].  q / k: bf16 tensors read in place through
    (batch, head, row) element strides; token_sets: B iterables of token indices below Nk (<= 128).  accumulate: add to `out` (which must be given)."""
    _chk(q, BF16, "attention_token_map.q")
    _chk(k, BF16, "attention_token_map.k")
    if Nk < 1 or Nk > TOKEN_MAP_MAX_KEYS or D % 8 or not 0 < D <= TOKEN_MAP_MAX_DIM or not 1 <= B <= MUTUAL_MAX_BATCH or N < 1 or H < 1:
        raise ValueError(f"attention_token_map: Nk <= {TOKEN_MAP_MAX_KEYS}, head dims that are multiples of 8 up to {TOKEN_MAP_MAX_DIM} and B <= "
                         f"{MUTUAL_MAX_BATCH} are covered, got B={B} H={H} N={N} Nk={Nk} D={D}")
    token_sets = [tuple(int(t) for t in s) for s in token_sets]
    if len(token_sets) != B or any(t >= Nk for s in token_sets for t in s):
        raise ValueError(f"attention_token_map: need {B} token sets with indices below Nk={Nk}, got {token_sets}")
    if accumulate and out is None:
        raise ValueError("attention_token_map: accumulate needs the buffer to add to")
    out = _out_buf(out, torch.float32, (B, N), "attention_token_map.out", q.device)
    words = [w for s in token_sets for w in token_set_words(s)]
    arr = (ctypes.c_ulonglong * (2 * B))(*words)
    check(lib.ae_attn_token_map_bf16(_p(q), _p(k), _p(out), B, H, N, Nk, D, *q_strides, *k_strides, float(scale), arr, 1 if accumulate else 0, _s()),
          "ae_attn_token_map_bf16")
    return out


def masactrl_classes(maps, S, R, thres, pairs, cls, counts):
    """Min-max normalisation, nearest resize S x S -> R x R (F.interpolate's index rule) and `>= thres` of several maps in one launch, without a
    read-back (ae_masactrl_classes).  maps: fp32 [B, S*S] contiguous; pairs: [(sample, out_row), ...] (1 .. 8); cls: uint8 [rows, R*R] and counts: int32
    [rows, 2] (zeros, ones per written row), both contiguous.  A constant map gives all-zero classes.  Returns (cls, counts)."""
    _chk(maps, torch.float32, "masactrl_classes.maps", 2)
    if S < 1 or R < 1 or maps.shape[1] != S * S or not maps.is_contiguous():
        raise ValueError(f"masactrl_classes.maps: expected contiguous fp32 [B, {S * S}] maps, got {tuple(maps.shape)}")
    pairs = [(int(s), int(o)) for s, o in pairs]
    _chk(cls, torch.uint8, "masactrl_classes.cls", 2)
    _chk(counts, torch.int32, "masactrl_classes.counts", 2)
    rows = cls.shape[0]
    if cls.shape[1] != R * R or not cls.is_contiguous() or tuple(counts.shape) != (rows, 2) or not counts.is_contiguous():
        raise ValueError(f"masactrl_classes: cls must be contiguous uint8 [rows, {R * R}] and counts int32 [rows, 2], got {tuple(cls.shape)} and "
                         f"{tuple(counts.shape)}")
    if not 1 <= len(pairs) <= MASACTRL_MAX_PAIRS or any(not 0 <= s < maps.shape[0] or not 0 <= o < rows for s, o in pairs):
        raise ValueError(f"masactrl_classes: 1 .. {MASACTRL_MAX_PAIRS} (sample, out_row) pairs inside the buffers are covered, got {pairs}")
    sa = (ctypes.c_int * len(pairs))(*(s for s, _ in pairs))
    oa = (ctypes.c_int * len(pairs))(*(o for _, o in pairs))
    check(lib.ae_masactrl_classes(_p(maps), maps.stride(0), S, R, float(thres), len(pairs), sa, oa, _p(cls), _p(counts), _s()), "ae_masactrl_classes")
    return cls, counts


# --------------------------------------------------------------------------- Prompt-to-Prompt attention control (csrc/prompt2prompt.hip)
P2P_HEAD_DIMS = (40, 64, 80, 160)
P2P_MAX_BATCH = 64
P2P_MAX_KEYS = 128
P2P_BLEND_MAX_LAYERS, P2P_BLEND_MAX_SIDE = 8, 32


def attention_p2p(q, k, v, B, H, N, Nk, D, scale, q_strides, k_strides, v_strides, base, M=None, c=None, d=None, store=None, store_row=None,
                  accumulate=False, out=None, o_strides=None, want_out=True):
    """Short-key cross-attention in which an edited sample's probabilities come from its base sample's (ae_attn_p2p_bf16).  q / k / v: bf16 tensors
    addressed via (batch, head, row) element strides, as `attention` takes them.  base: B host ints; base[b] == b: unedited, P' = softmax(q_b k_b^T);
    otherwise P' = (P_base M[b]) * c[b] + P_own * d[b], not renormalised.  M fp32 [B, Nk, Nk] contiguous or None (= the identity for every sample);
    c, d fp32 [B, Nk] contiguous (needed when any sample is edited).  store fp32 [rows, N, Nk] contiguous with store_row (B host ints, -1 = not
    stored): store[store_row[b]] (+)= sum over heads of P'[b] (accumulate: add).  want_out=False: no PV product, only the store is written (v may be
    None) and None is returned; otherwise out: [B, N, H*D] bf16."""
    _chk(q, BF16, "attention_p2p.q")
    _chk(k, BF16, "attention_p2p.k")
    if D not in P2P_HEAD_DIMS or not 1 <= Nk <= P2P_MAX_KEYS or not 1 <= B <= P2P_MAX_BATCH or N < 1 or H < 1:
        raise ValueError(f"attention_p2p: head dims {P2P_HEAD_DIMS}, Nk <= {P2P_MAX_KEYS} and B <= {P2P_MAX_BATCH} are covered, got B={B} H={H} N={N} "
                         f"Nk={Nk} D={D}")
    base = tuple(int(s) for s in base)
    if len(base) != B or any(s < 0 or s >= B for s in base):
        raise ValueError(f"attention_p2p: base needs {B} sample indices in [0, {B}), got {base}")
    if any(base[s] != s for s in base):
        raise ValueError(f"attention_p2p: a base sample must be unedited (base[base[b]] == base[b]), got {base}")
    edited = any(s != b for b, s in enumerate(base))
    if M is not None:
        _chk(M, torch.float32, "attention_p2p.M", 3)
        if tuple(M.shape) != (B, Nk, Nk) or not M.is_contiguous():
            raise ValueError(f"attention_p2p.M: expected a contiguous fp32 [{B}, {Nk}, {Nk}] tensor, got {tuple(M.shape)}")
    if edited and (c is None or d is None):
        raise ValueError("attention_p2p: an edited sample needs c and d")
    for t, n in ((c, "c"), (d, "d")):
        if t is not None:
            _chk(t, torch.float32, "attention_p2p." + n, 2)
            if tuple(t.shape) != (B, Nk) or not t.is_contiguous():
                raise ValueError(f"attention_p2p.{n}: expected a contiguous fp32 [{B}, {Nk}] tensor, got {tuple(t.shape)}")
    rows, rarr = 0, None
    if store is not None:
        _chk(store, torch.float32, "attention_p2p.store", 3)
        rows = store.shape[0]
        if tuple(store.shape[1:]) != (N, Nk) or not store.is_contiguous():
            raise ValueError(f"attention_p2p.store: expected a contiguous fp32 [rows, {N}, {Nk}] tensor, got {tuple(store.shape)}")
        if store_row is None:
            raise ValueError("attention_p2p: a store needs store_row")
        store_row = tuple(int(r) for r in store_row)
        kept = [r for r in store_row if r >= 0]
        if len(store_row) != B or any(r < -1 or r >= rows for r in store_row) or len(set(kept)) != len(kept):
            raise ValueError(f"attention_p2p: store_row needs {B} distinct rows in [0, {rows}) or -1, got {store_row}")
        rarr = (ctypes.c_int * B)(*store_row)
    elif store_row is not None or accumulate:
        raise ValueError("attention_p2p: store_row / accumulate without a store")
    if want_out:
        _chk(v, BF16, "attention_p2p.v")
        if out is None:
            out = torch.empty(B, N, H * D, dtype=BF16, device=q.device)
        else:
            _chk(out, BF16, "attention_p2p.out")
        if o_strides is None:
            o_strides = (N * H * D, D, H * D)
    else:
        if store is None:
            raise ValueError("attention_p2p: want_out=False needs a store to write")
        out, o_strides = None, (0, 0, 0)
        if v is None:
            v_strides = (0, 0, 0)
    barr = (ctypes.c_int * B)(*base)
    check(lib.ae_attn_p2p_bf16(_p(q), _p(k), _p(v), _p(out), B, H, N, Nk, D, *q_strides, *k_strides, *v_strides, *o_strides, float(scale), barr, _p(M),
                               _p(c), _p(d), _p(store), rarr, rows, 1 if accumulate else 0, _s()), "ae_attn_p2p_bf16")
    return out


def p2p_local_blend(maps, S, Nk, token_sets, threshold, x, out=None):
    """LocalBlend.__call__ in one launch with no read-back (ae_p2p_local_blend_f32).  maps: 1 .. 8 fp32 [2, S*S, Nk] contiguous store maps (head
    sums; any positive common factor is removed by the normalisation); token_sets: two iterables of token indices below Nk; x fp32 [2, C, h, w]
    contiguous.  mask_b = (resize(maxpool3x3(sum_layers sum_{j in set_b} map[b, :, j])) / its maximum) > threshold; out[1] = x[1] where mask_0 or
    mask_1, else x[0]; out[0] = x[0].  out: None (allocated), x itself (in place) or another fp32 [2, C, h, w] buffer."""
    maps = list(maps)
    if not 1 <= len(maps) <= P2P_BLEND_MAX_LAYERS or not 1 <= S <= P2P_BLEND_MAX_SIDE or not 1 <= Nk <= P2P_MAX_KEYS:
        raise ValueError(f"p2p_local_blend: 1 .. {P2P_BLEND_MAX_LAYERS} maps of side <= {P2P_BLEND_MAX_SIDE} with Nk <= {P2P_MAX_KEYS} are covered, "
                         f"got {len(maps)} maps, S={S}, Nk={Nk}")
    for i, m in enumerate(maps):
        _chk(m, torch.float32, f"p2p_local_blend.maps[{i}]", 3)
        if m.shape[0] != 2:
            raise ValueError(f"p2p_local_blend: exactly two samples (the reference's mask[:1] + mask[1:] broadcast holds for two prompts only), got "
                             f"maps[{i}] of shape {tuple(m.shape)}")
        if tuple(m.shape) != (2, S * S, Nk) or not m.is_contiguous():
            raise ValueError(f"p2p_local_blend.maps[{i}]: expected a contiguous fp32 [2, {S * S}, {Nk}] tensor, got {tuple(m.shape)}")
    _chk(x, torch.float32, "p2p_local_blend.x", 4)
    if x.shape[0] != 2:
        raise ValueError(f"p2p_local_blend: exactly two samples (the reference's mask[:1] + mask[1:] broadcast holds for two prompts only), got x of "
                         f"shape {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("p2p_local_blend.x: expected a contiguous tensor")
    token_sets = [tuple(int(t) for t in s) for s in token_sets]
    if len(token_sets) != 2 or any(t >= Nk for s in token_sets for t in s):
        raise ValueError(f"p2p_local_blend: need 2 token sets with indices below Nk={Nk}, got {token_sets}")
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, torch.float32, "p2p_local_blend.out", 4)
        if tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
            raise ValueError(f"p2p_local_blend.out: expected a contiguous fp32 {tuple(x.shape)} tensor, got {tuple(out.shape)}")
    words = [w for s in token_sets for w in token_set_words(s)]
    warr = (ctypes.c_ulonglong * 4)(*words)
    parr = (ctypes.c_void_p * len(maps))(*(m.data_ptr() for m in maps))
    _, C, h, w = x.shape
    check(lib.ae_p2p_local_blend_f32(parr, len(maps), S, Nk, warr, float(threshold), _p(x), _p(out), C, h, w, _s()), "ae_p2p_local_blend_f32")
    return out


def rows_to_nchw_out(x, out):
    """channels-last bf16 rows [B*H*W, C] contiguous -> the given [B, C, H, W] buffer (fp32 or bf16, contiguous): `rows_to_nchw` into a
    buffer the caller owns (no allocation)."""
    _chk(x, BF16, "rows_to_nchw_out.x", 2)
    if not out.is_cuda or out.dtype not in (torch.float32, BF16) or out.dim() != 4 or not out.is_contiguous():
        raise ValueError("rows_to_nchw_out: out must be a contiguous fp32 / bf16 [B, C, H, W] GPU tensor")
    B, C, H, W = out.shape
    if tuple(x.shape) != (B * H * W, C) or not x.is_contiguous():
        raise ValueError(f"rows_to_nchw_out: x must be a contiguous [{B * H * W}, {C}] buffer, got {tuple(x.shape)}")
    check(lib.ae_transpose_last2(_p(x), _p(out), B, H * W, C, H * W, 1, 1 if out.dtype == BF16 else 0, _s()), "ae_transpose_last2")
    return out


# --------------------------------------------------------------------------- layout / elementwise
def nchw_to_rows(x, c_pad=None):
    """[B,C,H,W] (fp32 or bf16) -> channels-last bf16 [B*H*W, Cpad] (zero padded channels)."""
    B, C, H, W = x.shape
    x = x.contiguous()
    c_pad = c_pad or C
    out = torch.empty(B * H * W, c_pad, dtype=BF16, device=x.device)
    check(lib.ae_transpose_last2(_p(x), _p(out), B, C, H * W, c_pad, 1 if x.dtype == BF16 else 0, 1, _s()), "ae_transpose_last2")
    return out


def rows_to_nchw(x, B, H, W, out_dtype=torch.float32):
    """channels-last [B*H*W, C] (bf16 or fp32) -> [B,C,H,W]."""
    if _TAPE is not None and _TAPE.active:
        return _TAPE.rows_to_nchw(x, B, H, W, out_dtype=out_dtype)
    C = x.shape[1]
    x = x.contiguous()
    out = torch.empty(B, C, H, W, dtype=out_dtype, device=x.device)
    check(lib.ae_transpose_last2(_p(x), _p(out), B, H * W, C, H * W, 1 if x.dtype == BF16 else 0,
                                 1 if out_dtype == BF16 else 0, _s()), "ae_transpose_last2")
    return out


def concat_channels(a, b):
    if _TAPE is not None and _TAPE.active:
        return _TAPE.concat_channels(a, b)
    a, b = _dense(a, BF16, "concat_channels.a", 2), _dense(b, BF16, "concat_channels.b", 2)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"concat_channels: {a.shape[0]} rows against {b.shape[0]}")
    out = torch.empty(a.shape[0], a.shape[1] + b.shape[1], dtype=BF16, device=a.device)
    check(lib.ae_concat_channels_bf16(_p(a), a.shape[1], _p(b), b.shape[1], _p(out), a.shape[0], _s()), "ae_concat_channels_bf16")
    return out


def split_channels(dy, ca, a=None, b=None, want_a=True, want_b=True):
    """Adjoint of `concat_channels`: (da, db) with da (+)= dy[:, :ca], db (+)= dy[:, ca:]; `a` / `b` are existing gradient
    buffers to add into (None: a fresh buffer is written).  One launch instead of two strided copies and two adds."""
    dy = _dense(dy, BF16, "split_channels.dy", 2)
    rows, C = dy.shape
    cb = C - ca
    if a is not None:
        _target(a, BF16, (rows, ca), "split_channels.a")
    if b is not None:
        _target(b, BF16, (rows, cb), "split_channels.b")
    da = a if a is not None else (torch.empty(rows, ca, dtype=BF16, device=dy.device) if want_a else None)
    db = b if b is not None else (torch.empty(rows, cb, dtype=BF16, device=dy.device) if want_b else None)
    check(lib.ae_split_channels_bf16(_p(dy), ca, cb, _p(da), _p(db), rows, int(a is not None), int(b is not None), _s()), "ae_split_channels_bf16")
    return da, db


def timestep_embedding(t, dim, max_period=10000.0, out_f32=False):
    B = t.shape[0]
    out = torch.empty(B, dim, dtype=torch.float32 if out_f32 else BF16, device=t.device)
    t_i64 = t if t.dtype == torch.int64 else None
    t_f32 = None if t_i64 is not None else t.float().contiguous()
    check(lib.ae_timestep_embedding(_p(t_i64), _p(t_f32), None if out_f32 else _p(out), _p(out) if out_f32 else None, B, dim,
                                    float(max_period), _s()), "ae_timestep_embedding")
    return out


def ddim_step(x, eps, coeffs, branches, s0=1.0, s1=0.0, noise=None, temperature=1.0, want_pred_x0=True, want_e=False):
    """coeffs = (sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef, sigma_t) as python floats holding fp32 values."""
    _chk(x, torch.float32, "ddim_step.x")
    _chk(eps, torch.float32, "ddim_step.eps")
    x = x.contiguous()
    eps = eps.contiguous()
    n = x.numel()
    if eps.numel() != branches * n:
        raise ValueError(f"ddim_step: eps has {eps.numel()} elements, expected {branches}*{n}")
    if noise is not None:
        noise = _dense(noise, torch.float32, "ddim_step.noise")
        if noise.numel() != n:
            raise ValueError(f"ddim_step: noise has {noise.numel()} elements, expected {n}")
    x_prev = torch.empty_like(x)
    pred_x0 = torch.empty_like(x) if want_pred_x0 else None
    s1m, sat, sap, dirc, sig = coeffs
    e_out = torch.empty_like(x) if want_e else None  # the guidance-combined eps (what PLMS keeps in its history)
    check(lib.ae_ddim_step_f32(_p(x), _p(eps), _p(noise), _p(x_prev), _p(pred_x0), _p(e_out), n, branches, s0, s1, s1m, sat, sap,
                               dirc, sig, temperature, _s()), "ae_ddim_step_f32")
    if want_e:
        return x_prev, pred_x0, e_out
    return x_prev, pred_x0


def ddim_encode_step(x, eps, cx, ce, branches=1, scale=1.0):
    """DDIM inversion update x_next = cx*x + ce*cfg(eps) (ddim.py:253-298); eps holds `branches` stacked predictions."""
    _chk(x, torch.float32, "ddim_encode_step.x")
    _chk(eps, torch.float32, "ddim_encode_step.eps")
    x, eps = x.contiguous(), eps.contiguous()
    out = torch.empty_like(x)
    check(lib.ae_ddim_encode_step_f32(_p(x), _p(eps), _p(out), x.numel(), branches, float(scale), float(cx), float(ce), _s()),
          "ae_ddim_encode_step_f32")
    return out


def dpm_multistep(x, model_out, branches, scale, sigma_s, alpha_s, predict_x0=True, v_param=False, m_prev=None, update=None,
                  want_m=True):
    """One DPM-Solver(++) multistep evaluation: returns (m, x_next).  update = (a, b, c, inv_r0) or None (history value only)."""
    _chk(x, torch.float32, "dpm_multistep.x")
    _chk(model_out, torch.float32, "dpm_multistep.model_out")
    n = x.numel()
    if model_out.numel() != branches * n or not x.is_contiguous() or not model_out.is_contiguous():
        raise ValueError("dpm_multistep: model_out must hold `branches` contiguous copies of x's shape")
    m = torch.empty_like(x) if want_m else None
    xn = torch.empty_like(x) if update is not None else None
    a, b, c, inv_r0 = update if update is not None else (0.0, 0.0, 0.0, 0.0)
    check(lib.ae_dpm_multistep_f32(_p(x), _p(model_out), _p(m_prev), _p(m), _p(xn), n, branches, float(scale), 1 if v_param else 0,
                                   1 if predict_x0 else 0, float(sigma_s), float(alpha_s), 1 if update is not None else 0, float(a),
                                   float(b), float(c), float(inv_r0), _s()), "ae_dpm_multistep_f32")
    return m, xn


def plms_combine(e_t, old_eps):
    """PLMS combination of e_t with the list of previous predictions (newest last, as plms.py keeps them); for the first step pass
    old_eps = [e_t_next] and order 0 via `plms_combine_first`."""
    order = min(len(old_eps), 3)
    e_t = e_t.contiguous()
    olds = [t.contiguous() for t in old_eps[::-1][:3]] + [None, None, None]
    out = torch.empty_like(e_t)
    check(lib.ae_plms_combine_f32(_p(e_t), _p(olds[0]), _p(olds[1]), _p(olds[2]), _p(out), e_t.numel(), order, _s()), "ae_plms_combine_f32")
    return out


def plms_combine_first(e_t, e_t_next):
    out = torch.empty(e_t.shape, dtype=e_t.dtype, device=e_t.device)   # contiguous like the kernel's view of the inputs (empty_like keeps a dense permuted layout)
    check(lib.ae_plms_combine_f32(_p(_tmp(e_t.contiguous())), _p(_tmp(e_t_next.contiguous())), None, None, _p(out), e_t.numel(), 0, _s()),
          "ae_plms_combine_f32")
    return out


def mask_blend_shape(mask, B, C, H, W):
    """How a mask broadcastable against [B, C, H, W] (the reference's `img_orig * mask + (1 - mask) * img`, ddim.py:154-157) is handed to
    the kernel, which reads one mask plane per sample: -> (mask expanded, samples, channels) with a per-channel mask ([B or 1, C, H, W])
    run as B*C single-channel samples."""
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    if mask.shape[1] == 1:
        return mask.expand(B, 1, H, W), B, C
    if mask.shape[1] == C:
        return mask.expand(B, C, H, W).reshape(B * C, 1, H, W), B * C, 1
    raise ValueError(f"mask_blend: mask of shape {tuple(mask.shape)} does not broadcast against [{B}, {C}, {H}, {W}]")


def mask_blend(img, x0, noise, mask, sqrt_ac, sqrt_one_minus_ac, ip2p_order=False):
    B, C, H, W = img.shape
    out = torch.empty(img.shape, dtype=img.dtype, device=img.device)   # the kernel writes row-major (not empty_like: see plms_combine_first)
    m, Bk, Ck = mask_blend_shape(mask, B, C, H, W)
    check(lib.ae_mask_blend_f32(_p(_tmp(img.contiguous())), _p(_tmp(x0.contiguous())), _p(_tmp(noise.contiguous())), _p(_tmp(m.contiguous().float())),
                                _p(out), Bk, Ck, H * W, sqrt_ac, sqrt_one_minus_ac, 1 if ip2p_order else 0, _s()), "ae_mask_blend_f32")
    return out


def q_sample(x0, noise, sqrt_ac_t, sqrt_one_minus_ac_t):
    """per-sample fp32 coefficient vectors [B] (already gathered at t)."""
    out = torch.empty(x0.shape, dtype=x0.dtype, device=x0.device)      # row-major (see plms_combine_first)
    B = x0.shape[0]
    check(lib.ae_q_sample_f32(_p(_tmp(x0.contiguous())), _p(_tmp(noise.contiguous())), _p(_tmp(sqrt_ac_t.contiguous())),
                              _p(_tmp(sqrt_one_minus_ac_t.contiguous())), _p(out), B, x0.numel() // B, _s()), "ae_q_sample_f32")
    return out


def silu_to_bf16(x):
    """silu(x) -> bf16 (ResBlock.emb_layers[0], openaimodel.py:212-214)."""
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(lib.ae_silu_to_bf16(_p(x), 1 if x.dtype == BF16 else 0, _p(out), x.numel(), _s()), "ae_silu_to_bf16")
    return out


def add_bcast(x, p):
    x, p = _dense(x, BF16, "add_bcast.x"), _dense(p, BF16, "add_bcast.p")
    out = torch.empty_like(x)
    check(lib.ae_add_bcast_bf16(_p(x), _p(p), _p(out), x.numel(), p.numel(), _s()), "ae_add_bcast_bf16")
    return out


def _no_tape(what):
    if _TAPE is not None and _TAPE.active:
        raise NotImplementedError(f"{what}: forward only (no backward closure on the tape; the AnyEdit training step never builds it)")


def resample2x_rows(x, B, H, W, down=False):
    """Channels-last rows [B*H*W, C] bf16 -> nearest x2 (Upsample(use_conv=False), openaimodel.py:108-118) or, down=True, the 2x2 mean of
    avg_pool_nd (Downsample(use_conv=False), :154-155).  Returns (rows, Ho, Wo)."""
    _no_tape("resample2x_rows")
    C = x.shape[1]
    if x.dtype != BF16 or not x.is_contiguous() or x.shape[0] != B * H * W or C % 8:
        raise ValueError(f"resample2x_rows: bf16 contiguous rows [B*H*W, C % 8 == 0] expected, got {tuple(x.shape)} {x.dtype}")
    Ho, Wo = (H // 2, W // 2) if down else (2 * H, 2 * W)
    out = torch.empty(B * Ho * Wo, C, dtype=BF16, device=x.device)
    check(lib.ae_resample2x_rows_bf16(_p(x), _p(out), B, H, W, C, 1 if down else 0, _s()), "ae_resample2x_rows_bf16")
    return out, Ho, Wo


def scale_shift_rows(x, emb, B, HW, silu=True):
    """ResBlock(use_scale_shift_norm=True), openaimodel.py:264-268: act(x * (1 + scale) + shift) over GroupNorm output rows x [B*HW, C] bf16; emb fp32
    [B, 2C] (rows may be strided: a column slice of the batched projection) = scale | shift."""
    _no_tape("scale_shift_rows")
    C = x.shape[1]
    if (x.dtype != BF16 or not x.is_contiguous() or x.shape[0] != B * HW or C % 8 or emb.dtype != torch.float32 or tuple(emb.shape) != (B, 2 * C)
            or emb.stride(1) != 1):
        raise ValueError(f"scale_shift_rows: x bf16 rows [B*HW, C % 8 == 0], emb fp32 [B, 2C] expected, got {tuple(x.shape)} {x.dtype} / {tuple(emb.shape)} {emb.dtype}")
    out = torch.empty_like(x)
    check(lib.ae_scale_shift_rows_bf16(_p(x), _p(emb), emb.stride(0), _p(out), B, HW, C, 1 if silu else 0, _s()), "ae_scale_shift_rows_bf16")
    return out


def window_partition(x, B, H, W, ws):
    C = x.shape[-1]
    nH, nW = (H + ws - 1) // ws, (W + ws - 1) // ws
    out = torch.empty(B * nH * nW * ws * ws, C, dtype=BF16, device=x.device)
    check(lib.ae_window_partition_bf16(_p(x), _p(out), B, H, W, C, ws, 0, _s()), "ae_window_partition_bf16")
    return out, (nH * ws, nW * ws)


def window_unpartition(windows, B, H, W, ws):
    C = windows.shape[-1]
    out = torch.empty(B * H * W, C, dtype=BF16, device=windows.device)
    check(lib.ae_window_partition_bf16(_p(out), _p(windows), B, H, W, C, ws, 1, _s()), "ae_window_partition_bf16")
    return out


def layernorm_window_ok(C):
    return bool(lib.ae_layernorm_window_supported(int(C)))


def _out_rows(out, rows, C, name):
    """`out`: None, or the caller's contiguous bf16 [rows, C] buffer the kernel writes to"""
    if out is not None and (out.dtype != BF16 or tuple(out.shape) != (rows, C) or not out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous bf16 [{rows}, {C}] tensor, got {tuple(out.shape)}")
    return out


def layernorm_window_partition(x, gamma, beta, eps, B, H, W, ws, out=None):
    """window_partition(LayerNorm(x)) in one launch (SAM Block norm1 + partition, image_encoder.py:166-173): x [B*H*W, C] image rows ->
    ([B*nH*nW*ws*ws, C] window rows with zero padding rows, (Hp, Wp))."""
    _chk(x, BF16, "layernorm_window_partition.x", 2)
    _chk(gamma, torch.float32, "layernorm_window_partition.gamma", 1)
    _chk(beta, torch.float32, "layernorm_window_partition.beta", 1)
    C = x.shape[1]
    if not x.is_contiguous() or x.shape[0] != B * H * W or gamma.numel() != C or beta.numel() != C:
        raise ValueError("layernorm_window_partition: x must be contiguous [B*H*W, C] rows, gamma / beta [C]")
    nH, nW = (H + ws - 1) // ws, (W + ws - 1) // ws
    out = _out_rows(out, B * nH * nW * ws * ws, C, "layernorm_window_partition")
    if out is None:
        out = torch.empty(B * nH * nW * ws * ws, C, dtype=BF16, device=x.device)
    check(lib.ae_layernorm_window_bf16(_p(x), None, _p(gamma), _p(beta), _p(out), None, B, H, W, C, ws, 1, eps, _s()),
          "ae_layernorm_window_bf16")
    return out, (nH * ws, nW * ws)


def window_merge_layernorm(windows, shortcut, gamma, beta, eps, B, H, W, ws, out=None, xsum_out=None):
    """(x, LayerNorm(x)) with x = shortcut + window_unpartition(windows) in one launch (SAM Block :175-181: un-partition, residual add, norm2)."""
    _chk(windows, BF16, "window_merge_layernorm.windows", 2)
    _chk(shortcut, BF16, "window_merge_layernorm.shortcut", 2)
    _chk(gamma, torch.float32, "window_merge_layernorm.gamma", 1)
    _chk(beta, torch.float32, "window_merge_layernorm.beta", 1)
    C = shortcut.shape[1]
    nwin_rows = B * ((H + ws - 1) // ws) * ((W + ws - 1) // ws) * ws * ws
    if not (windows.is_contiguous() and shortcut.is_contiguous()) or shortcut.shape[0] != B * H * W or tuple(windows.shape) != (nwin_rows, C) \
            or gamma.numel() != C or beta.numel() != C:
        raise ValueError("window_merge_layernorm: windows must be contiguous [B*nH*nW*ws*ws, C], shortcut [B*H*W, C], gamma / beta [C]")
    xsum, y = _out_rows(xsum_out, B * H * W, C, "window_merge_layernorm"), _out_rows(out, B * H * W, C, "window_merge_layernorm")
    xsum = torch.empty_like(shortcut) if xsum is None else xsum
    y = torch.empty_like(shortcut) if y is None else y
    check(lib.ae_layernorm_window_bf16(_p(windows), _p(shortcut), _p(gamma), _p(beta), _p(y), _p(xsum), B, H, W, C, ws, 2, eps, _s()),
          "ae_layernorm_window_bf16")
    return xsum, y


def sam_relpos_terms(q, q_strides, Rh, Rw, B, heads, qH, qW, D):
    Rh, Rw = _dense(Rh, torch.float32, "sam_relpos_terms.Rh", 3), _dense(Rw, torch.float32, "sam_relpos_terms.Rw", 3)
    kH, kW = Rh.shape[1], Rw.shape[1]
    rel_h = torch.empty(B * heads, qH * qW, kH, dtype=torch.float32, device=q.device)
    rel_w = torch.empty(B * heads, qH * qW, kW, dtype=torch.float32, device=q.device)
    check(lib.ae_sam_relpos_terms(_p(q), *q_strides, _p(Rh), _p(Rw), _p(rel_h), _p(rel_w), B, heads, qH, qW, kH, kW, D, _s()),
          "ae_sam_relpos_terms")
    return rel_h, rel_w


def softmax_rows(S, scale):
    """softmax(scale * S) over the last dim: fp32 [R, N] (row stride free) -> bf16 [R, N]."""
    _chk(S, torch.float32, "softmax_rows.S", 2)
    if S.stride(1) != 1 and S.shape[1] > 1:
        S = S.contiguous()
    out = torch.empty(S.shape, dtype=BF16, device=S.device)
    check(lib.ae_softmax_rows_f32_bf16(_p(S), S.stride(0), _p(out), out.stride(0), S.shape[0], S.shape[1], float(scale), _s()),
          "ae_softmax_rows_f32_bf16")
    return out


def gaussian_moments(moments, noise=None, want_stats=False):
    """DiagonalGaussianDistribution on moments [B, 2C, H, W] fp32: returns z (and mean, logvar, std if want_stats)."""
    moments = moments.float().contiguous()
    B, C2 = moments.shape[0], moments.shape[1]
    shape = (B, C2 // 2, *moments.shape[2:])
    z = torch.empty(shape, dtype=torch.float32, device=moments.device)
    stats = [torch.empty_like(z) for _ in range(3)] if want_stats else [None, None, None]
    if noise is not None:
        noise = noise.float().contiguous()
    check(lib.ae_gaussian_moments_f32(_p(moments), _p(noise), _p(z), _p(stats[0]), _p(stats[1]), _p(stats[2]), B, z.numel() // B, _s()),
          "ae_gaussian_moments_f32")
    return (z, *stats) if want_stats else z


def _msda_shapes(name, value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """Host-side shape comparisons only (no device read, so they hold under graph capture): the C entry sees raw pointers, and a
    mismatch would make the kernel read past a tensor.  -> (bs, S, heads, d, Q, L, P)"""
    bs, S, heads, d = value.shape
    if sampling_locations.dim() != 6 or sampling_locations.shape[-1] != 2:
        raise ValueError(f"{name}: sampling_locations must be [bs, Q, heads, L, P, 2], got {tuple(sampling_locations.shape)}")
    lb, Q, lh, L, P, _ = sampling_locations.shape
    if lb != bs or lh != heads:
        raise ValueError(f"{name}: sampling_locations {tuple(sampling_locations.shape)} are not of value's bs={bs}, heads={heads}")
    if tuple(attention_weights.shape) != (bs, Q, heads, L, P):
        raise ValueError(f"{name}: attention_weights {tuple(attention_weights.shape)} != {(bs, Q, heads, L, P)}")
    if tuple(spatial_shapes.shape) != (L, 2):
        raise ValueError(f"{name}: spatial_shapes {tuple(spatial_shapes.shape)} != {(L, 2)}")
    if tuple(level_start_index.shape) != (L,):
        raise ValueError(f"{name}: level_start_index {tuple(level_start_index.shape)} != {(L,)}")
    return bs, S, heads, d, Q, L, P


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=None, validated=False):
    """Drop-in for `_C.ms_deform_attn_forward` (GroundingDINO ms_deform_attn.py:42-60): value [bs, S, heads, d], spatial_shapes
    [L, 2] int64, level_start_index [L] int64, sampling_locations [bs, Q, heads, L, P, 2], attention_weights [bs, Q, heads, L, P]
    -> [bs, Q, heads*d] fp32.  `im2col_step` is accepted for signature compatibility (it only chunked the CUDA launch).
    `validated=True`: the caller has checked on the host that the levels add up to S (the check here reads the device tensor back, a
    synchronisation no graph capture allows)."""
    _chk(value, torch.float32, "ms_deform_attn.value", 4)
    bs, S, heads, d, Q, L, P = _msda_shapes("ms_deform_attn", value, spatial_shapes, level_start_index, sampling_locations, attention_weights)
    value = value.contiguous()
    loc = sampling_locations.float().contiguous()
    w = attention_weights.float().contiguous()
    shapes = spatial_shapes.to(torch.int64).contiguous()
    starts = level_start_index.to(torch.int64).contiguous()
    if not validated and int(shapes.prod(1).sum()) != S:
        raise ValueError("ms_deform_attn: spatial_shapes do not add up to value.shape[1]")
    out = torch.empty(bs, Q, heads * d, dtype=torch.float32, device=value.device)
    check(lib.ae_ms_deform_attn_fwd_f32(_p(value), _p(shapes), _p(starts), _p(loc), _p(w), _p(out), bs, S, heads, d, Q, L, P, _s()),
          "ae_ms_deform_attn_fwd_f32")
    return out


def ms_deform_attn_bwd(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, grad_output, im2col_step=None):
    """Drop-in for `_C.ms_deform_attn_backward` (GroundingDINO ms_deform_attn.py:68-90): returns (grad_value [bs, S, heads, d],
    grad_sampling_loc [bs, Q, heads, L, P, 2], grad_attn_weight [bs, Q, heads, L, P]), fp32."""
    _chk(value, torch.float32, "ms_deform_attn_bwd.value", 4)
    bs, S, heads, d, Q, L, P = _msda_shapes("ms_deform_attn_bwd", value, spatial_shapes, level_start_index, sampling_locations,
                                            attention_weights)
    value = value.contiguous()
    loc = sampling_locations.float().contiguous()
    w = attention_weights.float().contiguous()
    go = grad_output.float().contiguous()
    if tuple(go.shape) != (bs, Q, heads * d):
        raise ValueError(f"ms_deform_attn_bwd: grad_output {tuple(go.shape)} != {(bs, Q, heads * d)}")
    shapes = spatial_shapes.to(torch.int64).contiguous()
    starts = level_start_index.to(torch.int64).contiguous()
    gv, gl, gw = torch.empty_like(value), torch.empty_like(loc), torch.empty_like(w)
    check(lib.ae_ms_deform_attn_bwd_f32(_p(value), _p(shapes), _p(starts), _p(loc), _p(w), _p(go), _p(gv), _p(gl), _p(gw), bs, S, heads, d,
                                        Q, L, P, _s()), "ae_ms_deform_attn_bwd_f32")
    return gv, gl, gw


def linear_f32(x, w, bias=None):
    """nn.Linear in exact fp32 on the f32-input MFMA (ae_linear_f32): x [..., K] fp32, w [N, K] fp32, bias [N] -> [..., N] fp32.
    For layers the reference runs in fp32 and whose outputs are coordinates (GroundingDINO MSDeformAttn); K % 16 == 0."""
    _chk(x, torch.float32, "linear_f32.x")
    _chk(w, torch.float32, "linear_f32.w", 2)
    K = x.shape[-1]
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear_f32: x has {K} features, w has {w.shape[1]}")
    x2 = _tmp(x.reshape(-1, K).contiguous())
    w2 = _tmp(w.detach().contiguous())
    b2 = _tmp(bias.detach().float().contiguous()) if bias is not None else None
    M = x2.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    if M > 0:
        check(lib.ae_linear_f32(_p(x2), K, _p(w2), K, _p(b2), _p(out), N, M, N, K, _s()), "ae_linear_f32")
    return out.reshape(*x.shape[:-1], N)


def layernorm_act(x, gamma, beta, eps=1e-6, gelu=True, out=None):
    """LayerNorm over a narrow last dim (C <= 512) with fused GELU: the LayerNorm2d + GELU of the SAM mask decoder on rows."""
    _chk(x, BF16, "layernorm_act.x", 2)
    if not x.is_contiguous():
        raise ValueError("layernorm_act: x must be contiguous")
    M, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.ae_layernorm_act_bf16(_p(x), _p(gamma), _p(beta), _p(out), M, C, eps, 1 if gelu else 0, _s()), "ae_layernorm_act_bf16")
    return out


def sam_pe_encode(coords, gauss, image_size, labels=None, table=None, offset=0.5):
    """coords [N, 2] fp32 pixel (x, y); gauss [2, F] fp32; image_size (H, W).  -> [N, 2F] fp32 (prompt_encoder.py:73-102, 183-214)."""
    _chk(coords, torch.float32, "sam_pe_encode.coords", 2)
    _chk(gauss, torch.float32, "sam_pe_encode.gauss", 2)
    N, F = coords.shape[0], gauss.shape[1]
    if labels is not None:
        _chk(labels, torch.int32, "sam_pe_encode.labels", 1)
        _chk(table, torch.float32, "sam_pe_encode.table", 2)
        if table.shape != (5, 2 * F) or labels.shape[0] != N:
            raise ValueError("sam_pe_encode: table must be [5, 2F] and labels [N]")
    out = torch.empty(N, 2 * F, dtype=torch.float32, device=coords.device)
    if N == 0:
        return out
    check(lib.ae_sam_pe_encode_f32(_p(_tmp(coords.contiguous())), _p(labels), _p(_tmp(gauss.contiguous())), _p(table), _p(out), N, F, float(offset),
                                   1.0 / image_size[1], 1.0 / image_size[0], _s()), "ae_sam_pe_encode_f32")
    return out


def sam_mask_downscale(masks, w1, b1, g1, e1, w2, b2, g2, e2, eps=1e-6):
    """masks [B, 1, 4h, 4w] fp32 -> rows [B*h*w, 16] bf16 (PromptEncoder.mask_downscaling[0:6], mask_in_chans 16)."""
    _chk(masks, torch.float32, "sam_mask_downscale.masks", 4)
    B, one, H4, W4 = masks.shape
    if one != 1 or H4 % 4 or W4 % 4 or tuple(w1.shape) != (4, 1, 2, 2) or tuple(w2.shape) != (16, 4, 2, 2):
        raise ValueError("sam_mask_downscale: expects [B,1,4h,4w] masks and the mask_in_chans=16 weights")
    out = torch.empty(B * (H4 // 4) * (W4 // 4), 16, dtype=BF16, device=masks.device)
    check(lib.ae_sam_mask_downscale_bf16(_p(_tmp(masks.contiguous())), _p(w1), _p(b1), _p(g1), _p(e1), _p(w2), _p(b2), _p(g2), _p(e2), _p(out),
                                         B, H4 // 4, W4 // 4, eps, _s()), "ae_sam_mask_downscale_bf16")
    return out


def sam_mask_product(up, hyper, B, h, w):
    """up: bf16 rows [B*h*w*16, C] in un-shuffled (b, y, x, dy1, dx1, dy2, dx2) order; hyper [B, M, C] fp32 -> [B, M, 4h, 4w] fp32."""
    _chk(up, BF16, "sam_mask_product.up", 2)
    _chk(hyper, torch.float32, "sam_mask_product.hyper", 3)
    M, C = hyper.shape[1], hyper.shape[2]
    if up.shape != (B * h * w * 16, C) or not up.is_contiguous() or not hyper.is_contiguous() or hyper.shape[0] != B:
        raise ValueError("sam_mask_product: shape mismatch")
    out = torch.empty(B, M, 4 * h, 4 * w, dtype=torch.float32, device=up.device)
    check(lib.ae_sam_mask_product_f32(_p(up), _p(hyper), _p(out), B, h, w, M, C, _s()), "ae_sam_mask_product_f32")
    return out


def sam_postprocess_masks(low, img_size, input_size, original_size, threshold=None, want_logits=True, merge=False):
    """Sam.postprocess_masks fused (sam.py:133-162).  Returns (logits fp32 or None, bool mask or None).
    merge: the bool mask is the union over all B*M masks, shape [1, 1, oh, ow] (no logits)."""
    _chk(low, torch.float32, "sam_postprocess_masks.low", 4)
    B, M, Hl, Wl = low.shape
    oh, ow = int(original_size[0]), int(original_size[1])
    if merge and (threshold is None or want_logits):
        raise ValueError("sam_postprocess_masks: merge returns the thresholded union only (threshold required, want_logits=False)")
    logits = torch.empty(B, M, oh, ow, dtype=torch.float32, device=low.device) if want_logits else None
    mask = torch.empty((1, 1, oh, ow) if merge else (B, M, oh, ow), dtype=torch.uint8, device=low.device) if threshold is not None else None
    if B * M > 0:
        check(lib.ae_sam_postprocess_masks(_p(_tmp(low.contiguous())), _p(logits), _p(mask), B * M, Hl, Wl, int(img_size), int(input_size[0]),
                                           int(input_size[1]), oh, ow, float(threshold if threshold is not None else 0.0),
                                           1 if merge else 0, _s()), "ae_sam_postprocess_masks")
    elif mask is not None:
        mask.zero_()
    return logits, (mask.view(torch.bool) if mask is not None else None)


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: XYXY boxes [N, 4], scores [N] -> int64 indices of the kept boxes, by decreasing score."""
    if not boxes.is_cuda:
        raise ValueError("nms: expected GPU tensors (anyedit_amd has no CPU path)")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or scores.shape != boxes.shape[:1]:
        raise ValueError(f"nms: boxes must be [N, 4] and scores [N], got {tuple(boxes.shape)} / {tuple(scores.shape)}")
    N = boxes.shape[0]
    if N == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True).indices
    keep = torch.empty(N, dtype=torch.uint8, device=boxes.device)
    check(lib.ae_nms_sorted_f32(_p(_tmp(boxes.float()[order].contiguous())), _p(keep), N, float(iou_threshold), _s()), "ae_nms_sorted_f32")
    return order[keep.bool()]


def sam_preprocess(x, img_size, mean, std):
    """Sam.preprocess (sam.py:164-174): x [B, C, h, w] uint8 or fp32 -> normalised, zero-padded [B, C, S, S] fp32."""
    if x.dtype not in (torch.uint8, torch.float32):
        x = x.float()
    if not x.is_cuda:
        raise ValueError("sam_preprocess: expected a GPU tensor (anyedit_amd has no CPU path)")
    B, C, h, w = x.shape
    out = torch.empty(B, C, img_size, img_size, dtype=torch.float32, device=x.device)
    check(lib.ae_sam_preprocess_f32(_p(_tmp(x.contiguous())), 1 if x.dtype == torch.uint8 else 0, _p(out), B, C, h, w, img_size, _p(mean),
                                    _p(std), _s()), "ae_sam_preprocess_f32")
    return out


def patchify(x, P):
    B, Cin, H, W = x.shape
    out = torch.empty(B * (H // P) * (W // P), Cin * P * P, dtype=BF16, device=x.device)
    check(lib.ae_patchify_f32_bf16(_p(_tmp(x.float().contiguous())), _p(out), B, Cin, H, W, P, _s()), "ae_patchify_f32_bf16")
    return out


def lincomb(terms, out=None):
    """sum_i c_i * x_i over up to four (fp32 tensor, scalar) terms of one shape (ae_lincomb4_f32): the general DPM-Solver updates."""
    terms = [(t, float(c)) for t, c in terms if t is not None]
    if not 1 <= len(terms) <= 4:
        raise ValueError("lincomb: one to four terms")
    x0 = terms[0][0]
    for t, _ in terms:
        _chk(t, torch.float32, "lincomb.term")
        if t.shape != x0.shape or not t.is_contiguous():
            raise ValueError("lincomb: terms must be contiguous tensors of one shape")
    if out is None:
        out = torch.empty_like(x0)
    ptr = [(_p(t), c) for t, c in terms] + [(None, 0.0)] * (4 - len(terms))
    check(lib.ae_lincomb4_f32(_p(out), ptr[0][0], ptr[0][1], ptr[1][0], ptr[1][1], ptr[2][0], ptr[2][1], ptr[3][0], ptr[3][1], x0.numel(), _s()),
          "ae_lincomb4_f32")
    return out


def dpm_adaptive_err(x_lower, x_higher, x_prev, atol, rtol):
    """Per-sample error norm of the adaptive DPM-Solver (ae_dpm_adaptive_err_f32) -> fp32 [B]."""
    for t in (x_lower, x_higher, x_prev):
        _chk(t, torch.float32, "dpm_adaptive_err")
        if t.shape != x_lower.shape or not t.is_contiguous():
            raise ValueError("dpm_adaptive_err: contiguous tensors of one shape")
    B = x_lower.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=x_lower.device)
    check(lib.ae_dpm_adaptive_err_f32(_p(x_lower), _p(x_higher), _p(x_prev), float(atol), float(rtol), B, x_lower.numel() // B, _p(out), _s()),
          "ae_dpm_adaptive_err_f32")
    return out


def mse(a, b):
    ws = torch.empty(1 + 1024, dtype=torch.float32, device=a.device)    # the result and the per-block partial sums
    check(lib.ae_mse_f32(_p(_tmp(a.float().contiguous())), _p(_tmp(b.float().contiguous())), _p(ws), _p(ws[1:]), a.numel(), _s()), "ae_mse_f32")
    return ws[0]


def task_gate(task_emb, edit_code, Wg, bg):
    B = edit_code.shape[0]
    n_tasks, Dt = task_emb.shape
    E = Wg.shape[0]
    probs = torch.empty(B, E, dtype=torch.float32, device=task_emb.device)
    top1 = torch.empty(B, dtype=torch.int32, device=task_emb.device)
    top1p = torch.empty(B, dtype=torch.float32, device=task_emb.device)
    check(lib.ae_task_gate(_p(_tmp(task_emb.float().contiguous())), _p(_tmp(edit_code.long().contiguous())), _p(_tmp(Wg.float().contiguous())),
                           _p(_tmp(bg.float().contiguous())) if bg is not None else None, B, n_tasks, Dt, E, _p(probs), _p(top1),
                           _p(top1p), _s()), "ae_task_gate")
    return probs, top1, top1p


# --------------------------------------------------------------------------- per-op profiler (bench.py roofline leg)
# --------------------------------------------------------------------------- training-step kernels (row A11)
_TAPE = None  # set by anyedit_amd.autodiff.Tape while a differentiated forward is being recorded


def add(a, b, out=None):
    """a + b, bf16, same shape (gradient accumulation)."""
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.empty_like(a)
    check(lib.ae_add_bf16(_p(a), _p(b), _p(out), a.numel(), _s()), "ae_add_bf16")
    return out


def axpy(a, b, alpha=1.0, out=None):
    """a + alpha * b (bf16, same shape)."""
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.empty_like(a)
    check(lib.ae_axpy_bf16(_p(a), _p(b), float(alpha), _p(out), a.numel(), _s()), "ae_axpy_bf16")
    return out


def geglu(h):
    """h = [a | g] [M, 2F] bf16 -> a * gelu(g) [M, F] (attention.py:49-57, un-fused so that h is kept for the backward)."""
    if _TAPE is not None and _TAPE.active:
        return _TAPE.geglu(h)
    M, F2 = h.shape
    out = torch.empty(M, F2 // 2, dtype=BF16, device=h.device)
    check(lib.ae_geglu_fwd_bf16(_p(_tmp(h.contiguous())), _p(out), M, F2 // 2, _s()), "ae_geglu_fwd_bf16")
    return out


def geglu_bwd(h, dy):
    dh = torch.empty(h.shape, dtype=h.dtype, device=h.device)          # row-major like the kernel's view of h (see plms_combine_first)
    check(lib.ae_geglu_bwd_bf16(_p(_tmp(h.contiguous())), _p(_tmp(dy.contiguous())), _p(dh), h.shape[0], h.shape[1] // 2, _s()), "ae_geglu_bwd_bf16")
    return dh


def _grad_target(t, into):
    """`into`: a contiguous bf16 tensor of t's shape that already holds a gradient of t (the kernel then adds to it in place), or None."""
    if into is None:
        return torch.empty_like(t), 0
    if into.dtype != BF16 or into.shape != t.shape or not into.is_contiguous():
        raise ValueError("gradient accumulation target must be a contiguous bf16 tensor of the input's shape")
    return into, 1


def groupnorm_bwd(x, gamma, beta, dy, B, HW, eps, silu=False, groups=32, x2=None, stat=None, dx_into=None, dx2_into=None, dx_out=None, dx2_out=None):
    """dx_into / dx2_into: tensors that already hold a gradient of x / x2 — the kernel adds to them in place (no separate add launch) and they are returned.
    dx_out / dx2_out: the caller's buffers for a gradient that is written, not added (not together with the `_into` of the same tensor)."""
    C1 = x.shape[1]
    C = C1 + (x2.shape[1] if x2 is not None else 0)
    if (dx_into is not None and dx_out is not None) or (dx2_into is not None and dx2_out is not None):
        raise ValueError("groupnorm_bwd: a gradient is either added to `_into` or written to `_out`")
    dx, acc1 = _grad_target(x, dx_into) if dx_out is None else (_grad_target(x, dx_out)[0], 0)
    dx2, acc2 = (_grad_target(x2, dx2_into) if dx2_out is None else (_grad_target(x2, dx2_out)[0], 0)) if x2 is not None else (None, 0)
    ws = torch.empty(lib.ae_groupnorm_bwd_workspace_floats(B, HW, C, groups), dtype=torch.float32, device=x.device)
    check(lib.ae_groupnorm_bwd_nhwc_bf16(_p(x), _p(x2), C1, _p(gamma), _p(beta), _p(_tmp(dy.contiguous())), _p(dx), _p(dx2), B, HW, C, groups,
                                         eps, 1 if silu else 0, _p(ws), _p(_gn_counters(x.device, B)), _p(stat), acc1 | (acc2 << 1), _s()), "ae_groupnorm_bwd_nhwc_bf16")
    return dx, dx2


def layernorm_bwd(x, gamma, dy, eps=1e-5, want_param_grads=False, dx_into=None, dx_out=None, dgamma_out=None, dbeta_out=None):
    """dx_into: added to in place; dx_out / dgamma_out / dbeta_out: the caller's buffers (bf16 like x; fp32 [C]) for results that are written."""
    M, C = x.shape
    if dx_into is not None and dx_out is not None:
        raise ValueError("layernorm_bwd: the gradient is either added to dx_into or written to dx_out")
    dx, acc = _grad_target(x, dx_into) if dx_out is None else (_grad_target(x, dx_out)[0], 0)
    stat = torch.empty(M, 2, dtype=torch.float32, device=x.device) if want_param_grads else None
    dy = dy.contiguous()
    check(lib.ae_layernorm_bwd_bf16(_p(x), _p(gamma), _p(dy), _p(dx), _p(stat), M, C, eps, acc, _s()), "ae_layernorm_bwd_bf16")
    if not want_param_grads:
        return dx, None, None
    for t in (dgamma_out, dbeta_out):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (C,) or not t.is_contiguous()):
            raise ValueError("layernorm_bwd: dgamma_out / dbeta_out must be contiguous fp32 [C] tensors")
    dg = torch.empty(C, dtype=torch.float32, device=x.device) if dgamma_out is None else dgamma_out
    db = torch.empty(C, dtype=torch.float32, device=x.device) if dbeta_out is None else dbeta_out
    check(lib.ae_layernorm_param_grad_f32(_p(x), _p(dy), _p(stat), _p(dg), _p(db), M, C, _s()), "ae_layernorm_param_grad_f32")
    return dx, dg, db


def sumpool2x2(x, B, H, W):
    """x: [B*2H*2W, C] -> [B*H*W, C] (adjoint of the nearest-x2 upsample)."""
    out = torch.empty(B * H * W, x.shape[1], dtype=BF16, device=x.device)
    check(lib.ae_sumpool2x2_bf16(_p(_tmp(x.contiguous())), _p(out), B, H, W, x.shape[1], _s()), "ae_sumpool2x2_bf16")
    return out


def colsum(x):
    _chk(x, BF16, "colsum.x", 2)
    if x.stride(1) != 1 and x.shape[1] > 1:
        x = x.contiguous()
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    check(lib.ae_colsum_bf16_f32(_p(x), _p(out), x.shape[0], x.shape[1], x.stride(0), _s()), "ae_colsum_bf16_f32")
    return out


def mse_grad(pred, target, loss_scale=1.0):
    pred, target = pred.contiguous(), target.contiguous()
    out = torch.empty_like(pred)
    check(lib.ae_mse_grad_f32(_p(pred), _p(target), _p(out), pred.numel(), float(loss_scale), _s()), "ae_mse_grad_f32")
    return out


def adamw_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    """In-place torch.optim.AdamW update of one fp32 parameter tensor."""
    for t in (param, grad, exp_avg, exp_avg_sq):
        _chk(t, torch.float32, "adamw")
        if not t.is_contiguous():
            raise ValueError("adamw_step: tensors must be contiguous")
    check(lib.ae_adamw_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, betas[0], betas[1], eps, weight_decay,
                           int(step), float(grad_scale), _s()), "ae_adamw_f32")


def rowsum_f32(x):
    """x [R, n] fp32 -> [R] (fixed-order sums)."""
    x = x.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(lib.ae_rowsum_f32(_p(x), _p(out), x.shape[0], x.shape[1], _s()), "ae_rowsum_f32")
    return out


def scatter_add_rows(src, code, dst):
    """dst[code[b]] += src[b] (fp32), deterministic."""
    code = code.to(torch.int32).contiguous()
    check(lib.ae_scatter_add_rows_f32(_p(_tmp(src.contiguous())), _p(code), _p(dst), src.shape[0], src.shape[1], dst.shape[0], _s()),
          "ae_scatter_add_rows_f32")
    return dst


def task_gate_bwd(probs, top1, dgate, Wg):
    B, E = probs.shape
    dte = torch.empty(B, Wg.shape[1], dtype=torch.float32, device=probs.device)
    check(lib.ae_task_gate_bwd(_p(_tmp(probs.contiguous())), _p(_tmp(top1.contiguous())), _p(_tmp(dgate.float().contiguous())), _p(_tmp(Wg.float().contiguous())),
                               B, Wg.shape[1], E, _p(dte), _s()), "ae_task_gate_bwd")
    return dte


def task_gate_wgrad(probs, top1, dgate, task_emb, edit_code):
    """(dWg [E, Dt], dbg [E]) of the routed gate value (router parameters of the AnySD spec)."""
    B, E = probs.shape
    n_tasks, Dt = task_emb.shape
    probs32, top1c, dg32 = probs.float().contiguous(), top1.contiguous(), dgate.float().contiguous()
    te32, code = task_emb.float().contiguous(), edit_code.long().contiguous()
    dW = torch.empty(E, Dt, dtype=torch.float32, device=probs.device)
    db = torch.empty(E, dtype=torch.float32, device=probs.device)
    check(lib.ae_task_gate_wgrad(_p(probs32), _p(top1c), _p(dg32), _p(te32), _p(code), B, n_tasks, Dt, E, _p(dW), _p(db), _s()),
          "ae_task_gate_wgrad")
    return dW, db


_EXPERT_KV_WS = {}


def _experts_i32(experts):
    return experts.to(torch.int32).contiguous()


def expert_kv(x, W, experts, tokens):
    """kv[b*T+t] = x[b*T+t] @ bf16(W[experts[b]])^T for every sample in ONE launch (training forward of the AnySD adapters).
    x [B*T, Dc] bf16, W [E, N, Dc] fp32 master, experts [B] int -> [B*T, N] bf16."""
    E, N, Dc = W.shape
    B = x.shape[0] // tokens
    assert x.dtype == BF16 and x.is_contiguous() and W.dtype == torch.float32 and W.is_contiguous() and x.shape == (B * tokens, Dc)
    ex = _tmp(_experts_i32(experts))
    y = torch.empty(B * tokens, N, dtype=BF16, device=x.device)
    check(lib.ae_expert_kv_fwd(_p(x), _p(W), _p(ex), _p(y), B, tokens, N, Dc, E, _s()), "ae_expert_kv_fwd")
    return y


def expert_kv_dgrad(dy, W, experts, tokens):
    """dx[b*T+t] = dy[b*T+t] @ bf16(W[experts[b]]) (bf16), fixed summation order."""
    E, N, Dc = W.shape
    B = dy.shape[0] // tokens
    assert dy.dtype == BF16 and dy.is_contiguous() and dy.shape == (B * tokens, N)
    S = lib.ae_expert_kv_dgrad_slices(N)
    key = (dy.device, torch.cuda.current_stream(dy.device).cuda_stream)
    need = S * B * tokens * Dc
    ws = _EXPERT_KV_WS.get(key)
    if ws is None or ws.numel() < need:   # grow-only scratch per (device, stream): launches on a stream are ordered
        ws = _EXPERT_KV_WS[key] = torch.empty(need, dtype=torch.float32, device=dy.device)
    ex = _tmp(_experts_i32(experts))
    dx = torch.empty(B * tokens, Dc, dtype=BF16, device=dy.device)
    check(lib.ae_expert_kv_dgrad(_p(dy), _p(W), _p(ex), _p(dx), B, tokens, N, Dc, E, _p(ws), _s()), "ae_expert_kv_dgrad")
    return dx


def expert_kv_wgrad(dy, x, experts, tokens, n_experts, out=None):
    """dW[e] = sum over the samples routed to e of dy[b]^T x[b] (fp32 [E, N, Dc]; zeros for experts nothing was routed to)."""
    B = dy.shape[0] // tokens
    N, Dc = dy.shape[1], x.shape[1]
    assert dy.dtype == BF16 and x.dtype == BF16 and dy.is_contiguous() and x.is_contiguous()
    if out is None:
        out = torch.empty(n_experts, N, Dc, dtype=torch.float32, device=dy.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n_experts * N * Dc
    ex = _tmp(_experts_i32(experts))
    check(lib.ae_expert_kv_wgrad(_p(dy), _p(x), _p(ex), _p(out), B, tokens, N, Dc, n_experts, _s()), "ae_expert_kv_wgrad")
    return out


class OpProfiler:
    """Records (kernel label, algorithmic flops, algorithmic bytes, HIP-event duration) for every GEMM / conv / attention /
    norm launch issued through this module while active.  Events are recorded on torch's current stream, which is the
    stream the kernels are launched on."""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _PROF
        _PROF = self
        return self

    def __exit__(self, *a):
        global _PROF
        _PROF = None
        torch.cuda.synchronize()

    def summary(self, by_shape=False):
        agg = {}
        for label, flops, nbytes, e0, e1, nlaunch in self.records:
            if not by_shape:
                label = label.split("|")[0]
            ms = e0.elapsed_time(e1)
            a = agg.setdefault(label, {"calls": 0, "launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            a["calls"] += 1
            a["launches"] += nlaunch   # kernel launches behind the call (GroupNorm: 1-3, split-K conv: + the reduce; mirrors of the C launchers)
            a["ms"] += ms
            a["flops"] += flops
            a["bytes"] += nbytes
        for a in agg.values():
            a["avg_us"] = 1e3 * a["ms"] / a["calls"]
            a["tflops"] = a["flops"] / (a["ms"] * 1e-3) / 1e12 if a["ms"] > 0 else 0.0
            a["gbps"] = a["bytes"] / (a["ms"] * 1e-3) / 1e9 if a["ms"] > 0 else 0.0
        return agg


_PROF = None


def _wrap_profiled(fn, label_fn):
    def wrapped(*args, **kwargs):
        if _PROF is None:
            return fn(*args, **kwargs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kwargs)
        e1.record()
        lab = label_fn(out, *args, **kwargs)
        if lab is not None:   # None: an inner wrapped launch already recorded this call
            _PROF.records.append((lab[0], lab[1], lab[2], e0, e1, lab[3] if len(lab) > 3 else 1))
        return out
    wrapped.__doc__ = fn.__doc__
    return wrapped


def _gemm_label(_r, a, w, bias=None, residual=None, addvec=None, rows_per_batch=0, epilogue=EPI_NONE, out_f32=False, a2=None, **_):
    if _.get("rowstats") is not None:
        return None   # recorded by _gemm_ln_launch as "...,rowstats"
    M, (N, K) = a.shape[0], w.shape
    nb = 2 * (M * K + N * K) + _r.numel() * _r.element_size() + (2 * M * N if residual is not None else 0)
    if a2 is None and addvec is None and not out_f32 and _rowpanel_ok(a, w, _r, residual, M, N, K, epilogue):
        return f"gemm_rowpanel_kernel<K=320{',geglu' if epilogue == EPI_GEGLU else ''}>|M={M} N={N}", 2.0 * M * N * K, nb
    p = gemm_plan(M, N, K, epilogue, a.shape[1] if a2 is not None else 0, out_f32, _.get("colstats") is not None)
    return f"gemm_kernel<{plan_label(p)},dense>|M={M} N={N} K={K}", 2.0 * M * N * K, float(nb), 1 + p.colstats


def _conv_label(_r, x, w, bias, B, H, W, addvec=None, residual=None, stride=1, upsample2x=False, out_f32=False, **_):
    y = _r[0]
    M, Cout, Cin = y.shape[0], w.shape[0], x.shape[1]
    nb = 2 * (x.numel() + 9 * Cin * Cout) + y.numel() * y.element_size() + (2 * y.numel() if residual is not None else 0)
    p = conv_plan(B, H, W, Cin, Cout, stride, upsample2x, out_f32, _.get("colstats") is not None, _.get("k_order", 0))
    return f"gemm_kernel<{plan_label(p)},conv3x3>|M={M} Cin={Cin} Cout={Cout} s{stride}{'u' if upsample2x else ''}", 2.0 * M * Cout * 9 * Cin, float(nb), 1 + p.reduce + p.colstats


def _attn_label(_r, q, k, v, B, H, Nq, Nk, D, *a, **kw):
    # mirror of ae_attn_fast_launch: attention_fast.hip takes head dims 40 / 80 / 160 without key mask (rel-pos bias at d = 80 only, in its
    # kW == 64 or small-window forms); with <= 128 keys (and <= 64 in a second segment) its short-K/V variant runs
    fast = D in (40, 80, 160) and kw.get("key_mask") is None and os.environ.get("AE_ATTN_FAST", "1") != "0" and \
        (D != 160 or os.environ.get("AE_ATTN_FAST160", "1") != "0") and \
        (kw.get("rel_h") is None or (D == 80 and ((kw.get("kW") == 64 and Nk % 64 == 0) or (kw.get("kH", 99) <= 16 and kw.get("kW", 99) <= 16))))
    seg2 = kw.get("seg2")
    skv = fast and kw.get("rel_h") is None and Nk <= 128 and (seg2 is None or seg2[2] <= 64) and os.environ.get("AE_ATTN_SKV", "1") != "0"
    name = ("attn_fast_kernel" if fast else "attn_kernel")
    return f"{name}<D={D}{',shortKV' if skv else ''}>|Nq={Nq} Nk={Nk}", 4.0 * B * H * Nq * Nk * D, 2.0 * B * H * D * (2 * Nq + 2 * Nk)


def _attn8_label(_r, q, k, v, B, H, Nq, Nk, D, *a, **kw):
    return f"fp8_attn_kernel<D={D}>+prepare|Nq={Nq} Nk={Nk}", 4.0 * B * H * Nq * Nk * D, 2.0 * B * H * D * (2 * Nq + 2 * Nk)


def _gn_label(_r, x, gamma, beta, B, HW, eps, silu=False, groups=32, x2=None, **_):
    # launches behind the call (mirror of ae_groupnorm_nhwc_bf16): producer statistics -> finalize_cs + apply; maps up to 16x16 -> the one-launch
    # slab kernel; otherwise stats + finalize + apply (stats + apply with the last-block fold, AE_GN_TAIL)
    nl = 2 if _.get("colstats") is not None and ((x2 is None) == (_.get("colstats2") is None)) else (1 if HW <= 256 and os.environ.get("AE_GN_SLAB", "1") != "0" else (2 if _GN_TAIL else 3))
    return f"groupnorm(stats+apply)|rows={_r.shape[0]} C={_r.shape[1]}", 0.0, 2.0 * _r.numel() * 2, nl  # 1 read + 1 write algorithmic


def _ln_label(_r, x, *a, **_):
    return f"layernorm_kernel|M={_r.shape[0]} C={_r.shape[1]}", 0.0, 2.0 * _r.numel() * 2


def _ln_gemm_label(_r, x, w, bias, residual, gamma, beta, eps, epilogue, o, M, N, K, colstats=None):
    nb = 2 * (M * K + N * K) + _r.numel() * 2 + (2 * M * N if residual is not None else 0)
    return f"gemm_rowpanel_kernel<K=320,LN{',geglu' if epilogue == EPI_GEGLU else ''}>|M={M} N={N}", 2.0 * M * N * K, nb


def _gemm_ln_label(_r, a, w, bias, residual, epilogue, out, M, N, K, rowstats_out, ln_stats, nparts, ln_colsum, eps):
    nb = 2 * (M * K + N * K) + _r.numel() * 2 + (2 * M * N if residual is not None else 0)
    tag = "rowstats" if rowstats_out is not None else "LNfold"
    p = gemm_plan(M, N, K, epilogue, ln_mode=1 if rowstats_out is not None else 2)
    if p.rowpanel:   # round 5: the K = 320 shapes run the row-panel kernel's fold forms (ae_gemm_ln_bf16 forwards them)
        return f"gemm_rowpanel_kernel<K=320,{tag}{',geglu' if epilogue == EPI_GEGLU else ''}>|M={M} N={N}", 2.0 * M * N * K, nb
    return f"gemm_kernel<{plan_label(p)},dense,{tag}>|M={M} N={N} K={K}", 2.0 * M * N * K, float(nb)


def _up2_label(_r, x, w4, bias, B, H, W, **_):
    y = _r[0]
    Cout, Cin = w4.shape[1], x.shape[1]
    tl = plan_label(up2_plan(B, H, W, Cin, Cout, _.get("colstats") is not None))
    nb = 2 * (x.numel() + 16 * Cin * Cout) + 2 * y.numel()
    # FLOP: the 2x2 form's own count (4 taps per output pixel); the gather form it replaces spends 9/4 of it for the same function
    return f"gemm_kernel<{tl},conv3x3,up2x2>|M={y.shape[0]} Cin={Cin} Cout={Cout}", 2.0 * y.shape[0] * Cout * 4 * Cin, float(nb)


conv3x3_up2 = _wrap_profiled(conv3x3_up2, _up2_label)
ff_fused = _wrap_profiled(ff_fused, lambda _r, x, gamma, beta, eps, w1, b1, w2img, b2, residual=None, out=None, w3=None, b3=None, residual3=None, colstats=None: (
    f"ff_fused_kernel<C=320{',proj_out' if w3 is not None else ''}>|M={x.shape[0]} H={w1.shape[0] // 2}",
    2.0 * x.shape[0] * x.shape[1] * (3 * (w1.shape[0] // 2) + (x.shape[1] if w3 is not None else 0)),
    float(2 * (x.numel() * (2 + (residual is not None and residual is not x) + (residual3 is not None)) + w1.numel() + w2img.numel() + (w3.numel() if w3 is not None else 0))),
    2 if colstats is not None else 1))
_ln_gemm_fused = _wrap_profiled(_ln_gemm_launch, _ln_gemm_label)
_gemm_ln_launch = _wrap_profiled(_gemm_ln_launch, _gemm_ln_label)
gemm = _wrap_profiled(gemm, _gemm_label)
attention_fp8 = _wrap_profiled(attention_fp8, _attn8_label)
conv3x3 = _wrap_profiled(conv3x3, _conv_label)
attention = _wrap_profiled(attention, _attn_label)
groupnorm = _wrap_profiled(groupnorm, _gn_label)
layernorm = _wrap_profiled(layernorm, _ln_label)
expert_kv = _wrap_profiled(expert_kv, lambda _r, x, W, experts, tokens: (
    f"expert_kv_fwd_kernel|rows={x.shape[0]} N={W.shape[1]} Dc={W.shape[2]}", 2.0 * x.shape[0] * W.shape[1] * W.shape[2], 4.0 * (x.shape[0] // tokens) * W.shape[1] * W.shape[2]))
expert_kv_dgrad = _wrap_profiled(expert_kv_dgrad, lambda _r, dy, W, experts, tokens: (
    f"expert_kv_dgrad_kernel|rows={dy.shape[0]} N={W.shape[1]} Dc={W.shape[2]}", 2.0 * dy.shape[0] * W.shape[1] * W.shape[2], 4.0 * (dy.shape[0] // tokens) * W.shape[1] * W.shape[2]))
expert_kv_wgrad = _wrap_profiled(expert_kv_wgrad, lambda _r, dy, x, experts, tokens, n_experts, out=None: (
    f"expert_kv_wgrad_kernel|rows={dy.shape[0]} N={dy.shape[1]} Dc={x.shape[1]} E={n_experts}", 2.0 * dy.shape[0] * dy.shape[1] * x.shape[1], 4.0 * n_experts * dy.shape[1] * x.shape[1]))
hed_stem = _wrap_profiled(hed_stem, lambda _r, x, norm, w, bias, out=None: (
    f"hed_stem_kernel<{'u8' if x.dtype == torch.uint8 else 'f32'}>|M={_r[0].shape[0]} C1={_r[0].shape[1]}", 2.0 * 27 * _r[0].numel(),
    float(x.numel() * x.element_size() + 2 * _r[0].numel())))
relu_ = _wrap_profiled(relu_, lambda _r, x: (f"relu_bf16_kernel|n={x.numel()}", 0.0, 4.0 * x.numel()))
hed_tail = _wrap_profiled(hed_tail, lambda _r, y, wp, bp, B, H, W, pool=True, proj=None, pooled=None: (
    f"hed_tail_kernel<{'pool' if pool else 'last'}>|M={y.shape[0]} C={y.shape[1]}", 2.0 * y.numel(),
    float(2 * y.numel() + 4 * _r[0].numel() + (2 * _r[1].numel() if pool else 0))))
hed_fuse = _wrap_profiled(hed_fuse, lambda _r, sides, invert=True, out=None, logits=None, want_logits=False: (
    f"hed_fuse_kernel|B={sides[0].shape[0]} {sides[0].shape[-2]}x{sides[0].shape[-1]}", 0.0,
    float(4 * sum(s.numel() for s in sides) + sides[0].numel() * (1 + 4 * (want_logits or logits is not None)))))
dpt_reassemble = _wrap_profiled(dpt_reassemble, lambda _r, prod, bias, B, gh, gw, k, out=None: (
    f"dpt_reassemble_kernel<k={k}>|M={_r.shape[0]} oc={_r.shape[1]}", 0.0, 6.0 * _r.numel()))
dpt_resize = _wrap_profiled(dpt_resize, lambda _r, x, B, h, w, H, W, addend=None, out=None, relu_out=None, want_relu=False: (
    f"dpt_resize_kernel<{'add' if addend is not None else 'plain'}{'+relu' if want_relu or relu_out is not None else ''}>|{h}x{w}->{H}x{W} C={x.shape[1]}", 0.0,
    float(2 * x.numel() + 2 * B * H * W * x.shape[1] * (1 + (addend is not None) + (want_relu or relu_out is not None)))))
dpt_relu = _wrap_profiled(dpt_relu, lambda _r, x, out=None: (f"dpt_relu_kernel|n={x.numel()}", 0.0, 4.0 * x.numel()))
dpt_tail = _wrap_profiled(dpt_tail, lambda _r, y, wp, bp, B, H, W, out=None: (
    f"dpt_tail_kernel|M={y.shape[0]} C={y.shape[1]}", 2.0 * y.numel(), float(2 * y.numel() + 4 * y.shape[0])))
depth_resize_minmax = _wrap_profiled(depth_resize_minmax, lambda _r, depth, H, W, out=None, minmax=None: (
    f"depth_resize_minmax_kernel|B={depth.shape[0]} {depth.shape[1]}x{depth.shape[2]}->{H}x{W}", 0.0, float(4 * depth.numel() + 4 * _r[0].numel()), 2))
depth_colorize = _wrap_profiled(depth_colorize, lambda _r, depth, minmax, table, out=None: (
    f"depth_colorize_kernel|B={depth.shape[0]} {depth.shape[1]}x{depth.shape[2]}", 0.0, 7.0 * depth.numel()))
dwconv = _wrap_profiled(dwconv, lambda _r, x, w, bias, B, H, W, residual=None, out=None: (
    f"dwconv_rows_kernel<k={int(w.shape[0] ** 0.5 + 0.5)}{',res' if residual is not None else ''}>|B={B} {H}x{W} C={x.shape[1]}", 2.0 * w.shape[0] * x.numel(),
    float(2 * x.numel() * (2 + (residual is not None and residual is not x)) + 4 * w.numel())))   # algorithmic: x once, out once, a separate residual once
patch2_rows = _wrap_profiled(patch2_rows, lambda _r, x, B, H, W, out=None: (
    f"patch2_rows_kernel|B={B} {H}x{W} C={x.shape[1]}", 0.0, 4.0 * _r[0].numel()))
layernorm_rows_nchw = _wrap_profiled(layernorm_rows_nchw, lambda _r, x, gamma, beta, eps, B, H, W, out=None, rows=None, want_rows=False: (
    f"layernorm_rows_nchw_kernel{'<+rows>' if want_rows or rows is not None else ''}|B={B} {H}x{W} C={x.shape[1]}", 0.0,
    float(x.numel() * (2 + 4 + 2 * (want_rows or rows is not None)))))
ppm_pool = _wrap_profiled(ppm_pool, lambda _r, x, B, H, W, scales, out=None: (
    f"ppm_pool_kernel<{len(tuple(scales))} scales>|B={B} {H}x{W} C={x.shape[1]}", 0.0, float(2 * x.numel() * len(tuple(scales)) + 2 * _r.numel())))   # every scale reads the map once
resize_concat = _wrap_profiled(resize_concat, lambda _r, sources, dst, B, H, W, addend=None: (
    f"resize_concat_kernel<{len(sources)} sources{',add' if addend is not None else ''}>|->{H}x{W} ld={dst.shape[1]}", 0.0,
    float(sum(2 * s[0].numel() + 2 * B * H * W * s[0].shape[-1] for s in sources) + (2 * addend.numel() if addend is not None else 0))))
seg_argmax = _wrap_profiled(seg_argmax, lambda _r, logits, ncls, B, h, w, mid, out_size=None, palette=None, labels=None, colours=None: (
    f"seg_argmax_kernel<{'identity' if out_size is None or tuple(out_size) == tuple(mid) else 'two stages'}{',palette' if palette is not None else ''}>|{h}x{w}->{mid[0]}x{mid[1]} "
    f"ncls={ncls}", 0.0, float(4 * B * h * w * ncls + B * (out_size or mid)[0] * (out_size or mid)[1] * (4 if palette is not None else 1))))   # logits once, labels and colours once
