"""GPU tests of the DINOv2 image encoder: its two kernels against float64 between sentinel guards, both tiny towers against the reference's golden
at every stored image size and the full-width towers against the restatement (under the project's 1.5 x control rule), the LayerScale fold after
an in-place change, list inputs, the cached unconditional hint, batch independence, graph capture without allocations, and ControlLDM's
conditioning.  Every case runs once.

Two comparison rules.  Kernel rule: every element against float64 within 2^-8 |ref| + 1e-30 (one bf16 rounding).  Tower rule: err(HIP) <=
1.5 x err(bf16-storage control), both against the stored or fp32 reference."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import dino_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0x7FA5          # a NaN bit pattern no kernel writes
GUARD = 4096
TINY = {
    "swiglu": dict(embed_dim=128, num_heads=2, depth=2, patch_size=14, img_size=70, mlp_ratio=4.0, ffn_layer="swiglufused"),
    "mlp": dict(embed_dim=192, num_heads=3, depth=2, patch_size=14, img_size=56, mlp_ratio=2.0, ffn_layer="mlp"),
}
SIZES = {"swiglu": [(70, 70), (42, 42), (28, 42)], "mlp": [(56, 56), (84, 84)]}
PROJECTOR_OUT = 96
CASES = [(g, s) for g in TINY for s in SIZES[g]]
CASE_IDS = [f"{g}_{s[0]}x{s[1]}" for g, s in CASES]


def _guarded(shape):
    """A bf16 buffer of `shape` between two sentinel-filled guard bands, itself pre-filled with the sentinel."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, dtype=BF, device=DEV)
    buf.view(torch.int16).fill_(SENT)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    iv = buf.view(torch.int16)
    return bool((iv[:GUARD] == SENT).all()) and bool((iv[-GUARD:] == SENT).all())


def _twice(shape, launch):
    """Runs `launch(out)` twice on fresh guarded buffers: guards intact, the two results bit-identical; returns the result on the CPU."""
    bits = []
    for _ in range(2):
        buf, out = _guarded(shape)
        launch(out)
        torch.cuda.synchronize()
        assert _guards_intact(buf), "wrote outside its output"
        bits.append(out.clone().view(torch.int16).cpu())
    assert torch.equal(bits[0], bits[1]), "two launches differ"
    return bits[0].view(BF)


def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


def _kernel_ratio(got, ref):
    return float(((got.to(F64) - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-30)).max())


# ------------------------------------------------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", [1, 6, 256])
@pytest.mark.parametrize("C", [128, 384, 1536])
def test_dino_embed_vs_float64(C, G, B):
    """Kernel rule on every element; the patch product sits in a buffer whose row stride is wider than C (the pad holds NaN); the class rows,
    checked separately, are the same bits in every sample."""
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(C * 1000 + G * 10 + B)
    ldp = C + 12
    wide = torch.full((B * G, ldp), float("nan"))
    patch = torch.randn(B * G, C, generator=gen) * 0.7
    wide[:, :C] = patch
    bias, cls, pos = torch.randn(C, generator=gen) * 0.1, torch.randn(C, generator=gen), torch.randn(G + 1, C, generator=gen) * 0.3
    dw, db, dc, dp = (t.to(DEV) for t in (wide, bias, cls, pos))
    N = G + 1
    got = _twice((B * N, C), lambda out: ops.dino_embed(dw[:, :C], db, dc, dp, B, out=out)).view(B, N, C)
    ref_cls = cls.to(F64) + pos[0].to(F64)
    ref = patch.to(F64).view(B, G, C) + bias.to(F64) + pos[1:].to(F64)
    r_cls, r_patch = _kernel_ratio(got[:, 0], ref_cls.expand(B, C)), _kernel_ratio(got[:, 1:], ref)
    print(f"dino_embed C={C} G={G} B={B}: worst |err| / bound: class rows {r_cls:.3f}, patch rows {r_patch:.3f}")
    assert torch.isfinite(got.float()).all() and r_cls <= 1.0 and r_patch <= 1.0
    for b in range(1, B):
        assert torch.equal(got[b, 0], got[0, 0]), "the class row must not depend on the sample"


@pytest.mark.parametrize("Hd", [8, 344, 4096])
@pytest.mark.parametrize("M", [1, 10, 257])
def test_swiglu_vs_float64(M, Hd):
    """Kernel rule on every element, inputs from N(0, 3) so both tails of the sigmoid are reached; u with a row stride wider than 2 Hd (the pad
    holds NaN); once into a contiguous output, once into an output whose leading dimension is wider than Hd, whose pad columns must read zero."""
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(M * 10000 + Hd)
    ldu = 2 * Hd + 8
    wide = torch.full((M, ldu), float("nan"))
    u = torch.randn(M, 2 * Hd, generator=gen) * 3.0
    wide[:, :2 * Hd] = u
    bias = torch.randn(2 * Hd, generator=gen) * 3.0
    du, db = wide.to(DEV), bias.to(DEV)
    t = u.to(F64) + bias.to(F64)
    x1, x2 = t[:, :Hd], t[:, Hd:]
    ref = x1 * torch.sigmoid(x1) * x2
    assert float(x1.min()) < -6.0 and float(x1.max()) > 6.0 or M * Hd < 100
    got = _twice((M, Hd), lambda out: ops.swiglu(du[:, :2 * Hd], db, out=out))
    ratio = _kernel_ratio(got, ref)
    ldy = Hd + 24
    padded = _twice((M, ldy), lambda out: ops.swiglu(du[:, :2 * Hd], db, out=out[:, :Hd]))
    assert torch.equal(padded[:, :Hd].contiguous().view(torch.int16), got.view(torch.int16)), "the leading dimension changed the values"
    assert bool((padded[:, Hd:].view(torch.int16) == 0).all()), "pad columns must be written as zeros"
    print(f"swiglu M={M} Hd={Hd}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from anyedit_amd import ops, _lib
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(_lib.AnyEditHipError, match="multiple of 8"):
        ops.swiglu(z(2, 24), z(24))
    with pytest.raises(_lib.AnyEditHipError, match="multiple of 8"):
        ops.dino_embed(z(4, 12), z(12), z(12), z(5, 12), 1)
    with pytest.raises(ValueError, match="do not split"):
        ops.dino_embed(z(5, 16), z(16), z(16), z(3, 16), 2)
    with pytest.raises(ValueError, match="pos"):
        ops.dino_embed(z(4, 16), z(16), z(16), z(4, 16), 1)
    with pytest.raises(ValueError, match="out must be"):
        ops.swiglu(z(2, 32), z(32), out=z(2, 32, dt=BF))
    with pytest.raises(TypeError):
        ops.swiglu(z(2, 32, dt=BF), z(32))


# ------------------------------------------------------------------------------------------------------------ tiny towers vs golden
def _weights(geom):
    arrs = dict(load_golden(f"dino_tiny_{geom}_w0"), **load_golden(f"dino_tiny_{geom}_w1"))
    sd = sub_sd(arrs, "w.")
    proj = sub_sd(arrs, "e.")
    return sd, (dict({"model." + k: v for k, v in sd.items()}, **proj) if proj else None)


def _tiny(geom):
    from anyedit_amd.ldm.modules.encoders.dino_vision import DinoVisionTransformer
    sd, esd = _weights(geom)
    m = DinoVisionTransformer(dict(TINY[geom]))
    m.load_state_dict(sd)
    return m.to(DEV).eval().requires_grad_(False), sd, esd


def _tiny_encoder():
    from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder
    sd, esd = _weights("swiglu")
    e = FrozenDinoV2Encoder(dict(TINY["swiglu"]), projector_out=PROJECTOR_OUT)
    e.load_state_dict(esd)
    return e.to(DEV).eval().requires_grad_(False), esd


@pytest.mark.parametrize("geom,size", CASES, ids=CASE_IDS)
def test_tiny_tower_vs_reference_golden(geom, size):
    """Every stored output at this image size (the all-zero image is in its batch) under the tower rule, control = dino_ref(bf16_storage=True)
    on the same weights: through forward_features, through get_intermediate_layers with every combination of n / norm / return_class_token /
    reshape (what the fixture does not store — un-normed block 0 — is judged against the fp32 restatement the CPU suite pins to the fixture),
    through forward and, for swiglu, through FrozenDinoV2Encoder.encode.  28x42 pins the grid order of the interpolation."""
    m, sd, esd = _tiny(geom)
    o = load_golden(f"dino_tiny_{geom}_out_{size[0]}x{size[1]}")
    cfg = TINY[geom]
    heads, C, P = cfg["num_heads"], cfg["embed_dim"], cfg["patch_size"]
    gh, gw = size[0] // P, size[1] // P
    G = gh * gw
    px = T(o["pixels"])
    assert bool((px[2] == 0).all())
    ref = R.dino_forward(sd, px, heads)
    ctl = R.dino_forward(sd, px, heads, bf16_storage=True)
    report, ok = [], True
    pd = px.to(DEV)
    f = m.forward_features(pd)
    assert sorted(f) == ["masks", "x_norm_clstoken", "x_norm_patchtokens", "x_norm_regtokens", "x_prenorm"] and f["masks"] is None
    assert f["x_norm_clstoken"].shape == (3, C) and f["x_norm_patchtokens"].shape == (3, G, C) and f["x_prenorm"].shape == (3, G + 1, C)
    assert f["x_norm_regtokens"].shape == (3, 0, C) and all(f[k].dtype == BF for k in f if k != "masks")
    for name in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        ok &= _judge("forward_features()." + name, f[name], ctl[name], T(o[name]), report)
    ok &= _judge("forward()", m(pd), ctl["x_norm_clstoken"], T(o["x_norm_clstoken"]), report)
    for n, norm, rct, reshape in itertools.product(([0, 1], 1, 2, [0], [1]), (True, False), (True, False), (True, False)):
        got = m.get_intermediate_layers(pd, n=n, reshape=reshape, return_class_token=rct, norm=norm)
        want_c = R.intermediate_layers(ctl, n, gh, gw, reshape=reshape, return_class_token=True, norm=norm)
        want_r = R.intermediate_layers(ref, n, gh, gw, reshape=reshape, return_class_token=True, norm=norm)
        take = list(range(2 - n, 2)) if isinstance(n, int) else n
        assert isinstance(got, tuple) and len(got) == len(take)
        for j, i in enumerate(take):
            patch, cls = got[j] if rct else (got[j], None)
            assert patch.shape == ((3, C, gh, gw) if reshape else (3, G, C)) and patch.dtype == BF
            stored = norm                                                                       # the fixture holds the normed outputs of both blocks
            r_patch = T(o[f"inter.{i}.patch"]) if stored else want_r[j][0]
            if stored and reshape:
                r_patch = r_patch.reshape(3, gh, gw, C).permute(0, 3, 1, 2)
            if not stored and i == 1:
                r_patch = T(o["x_prenorm"])[:, 1:]
                r_patch = r_patch.reshape(3, gh, gw, C).permute(0, 3, 1, 2) if reshape else r_patch
            tag = f"get_intermediate_layers(n={n}, norm={norm}, cls={rct}, reshape={reshape})[{i}]"
            ok &= _judge(tag, patch, want_c[j][0], r_patch, report)
            if rct:
                r_cls = T(o[f"inter.{i}.cls"]) if stored else (T(o["x_prenorm"])[:, 0] if i == 1 else want_r[j][1])
                assert cls.shape == (3, C)
                ok &= _judge(tag + ".cls", cls, want_c[j][1], r_cls, report)
    if esd is not None:
        e, _ = _tiny_encoder()
        hint = e.encode(pd)
        assert hint.shape == (3, G + 1, PROJECTOR_OUT) and hint.dtype == BF
        ok &= _judge("FrozenDinoV2Encoder.encode()", hint, R.encoder_forward(esd, px, heads, bf16_storage=True), T(o["hint"]), report)
        assert torch.equal(e(pd), hint) and torch.equal(e.encode_pixels(pd), hint)
    print("\n".join(r for r in report if "get_intermediate" not in r or "ratio" in r))
    assert ok, "\n".join(report)


def test_list_input_unconditional_and_copies():
    """A list gives the same rows as the concatenated tensor; unconditional(3) equals encode of three zero images bit for bit and its second call
    launches nothing; encode returns a copy the caller owns."""
    e, esd = _tiny_encoder()
    px = T(load_golden("dino_tiny_swiglu_out_28x42")["pixels"]).to(DEV)
    whole = e.encode(px)
    parts = e.encode([px[:1].contiguous(), px[1:].contiguous()])
    assert torch.equal(whole, parts)
    assert torch.equal(e.model(px).clone(), e.model([px[:2].contiguous(), px[2:].contiguous()]))
    zeros = e.encode(torch.zeros(3, 3, 28, 42, device=DEV))
    assert torch.equal(whole[2], zeros[0])                                                       # the fixture's third image is all zero
    un = e.unconditional(3, size=(28, 42))
    assert torch.equal(un, zeros) and un.shape == (3, 7, PROJECTOR_OUT)
    from_list = e.encode([torch.zeros(1, 3, 28, 42)] * 3)                                         # the reference's own call: CPU zeros in a list
    assert torch.equal(from_list, un)
    torch.cuda.synchronize()
    static = e.encode_pixels(px)
    before = static.clone()
    launched = []
    from anyedit_amd import ops
    real = ops.gemm
    ops.gemm = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        again = e.unconditional(3, size=(28, 42))
    finally:
        ops.gemm = real
    assert again is un and not launched and torch.equal(static, before), "a cached unconditional hint must launch nothing"
    assert e.unconditional(1).shape == (1, 257, PROJECTOR_OUT)                                   # the reference's 224 x 224 zeros: 16 x 16 + 1 tokens
    assert whole.data_ptr() != static.data_ptr() and torch.equal(whole, before)


def test_layerscale_is_live():
    """Multiplying one block's ls2.gamma by 2 in place changes x_prenorm, and the result meets the tower rule against the restatement on the
    changed weights: the fold follows the parameters."""
    m, sd, _ = _tiny("swiglu")
    px = T(load_golden("dino_tiny_swiglu_out_42x42")["pixels"])
    pd = px.to(DEV)
    before = m.forward_features(pd)["x_prenorm"].clone()
    with torch.no_grad():
        m.blocks[0].ls2.gamma.mul_(2.0)
    sd2 = dict(sd)
    sd2["blocks.0.ls2.gamma"] = sd["blocks.0.ls2.gamma"] * 2.0
    after = m.forward_features(pd)
    assert not torch.equal(after["x_prenorm"], before)
    ref, ctl = R.dino_forward(sd2, px, 2), R.dino_forward(sd2, px, 2, bf16_storage=True)
    report, ok = [], True
    for name in ("x_prenorm", "x_norm_patchtokens", "x_norm_clstoken"):
        ok &= _judge("ls2 x 2: " + name, after[name], ctl[name], ref[name], report)
    stale = rel_l2(before.float().cpu(), ref["x_prenorm"])
    report.append(f"the stale fold would be at {stale:.3e}")
    print("\n".join(report))
    assert ok and stale > 10 * rel_l2(ctl["x_prenorm"], ref["x_prenorm"]), "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ full width, two blocks
@pytest.mark.parametrize("name", ["ViT-g", "ViT-L"])
def test_full_width_tower_vs_restatement(name):
    """The real geometry (224 px, 257 tokens, B = 2; the position table interpolated from 37 x 37 to 16 x 16 as in production) cut to two blocks,
    seeded weights, under the tower rule; for ViT-g also the projected hint [2, 257, 1024]."""
    from anyedit_amd.ldm.modules.encoders import dino_vision as dv
    vitg = name == "ViT-g"
    cfg = dict(dv.DINOV2_VITG14 if vitg else dv.DINOV2_VITL14, depth=2)
    sd = R.seeded_state_dict(cfg, seed=0, projector_out=1024 if vitg else None)
    with torch.device("meta"):
        m = dv.FrozenDinoV2Encoder(cfg) if vitg else dv.DinoVisionTransformer(cfg)
    m.load_state_dict(sd, assign=True)
    m = m.to(DEV)
    tower = m.model if vitg else m
    tsd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")} if vitg else sd
    px = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    heads = cfg["num_heads"]
    ref, ctl = R.dino_forward(tsd, px, heads), R.dino_forward(tsd, px, heads, bf16_storage=True)
    f = tower.forward_features(px.to(DEV))
    assert f["x_prenorm"].shape == (2, 257, cfg["embed_dim"]) and tower.pos_table(16, 16).shape == (257, cfg["embed_dim"])
    report, ok = [], True
    for key in ("x_prenorm", "x_norm_patchtokens", "x_norm_clstoken"):
        ok &= _judge(f"{name} {key}", f[key], ctl[key], ref[key], report)
    first = tower.get_intermediate_layers(px.to(DEV), n=[0], norm=False)[0]
    ok &= _judge(f"{name} block 0", first, ctl["hidden"][1][:, 1:], ref["hidden"][1][:, 1:], report)
    if vitg:
        hint = m.encode(px.to(DEV))
        assert hint.shape == (2, 257, 1024) and hint.dtype == BF
        ok &= _judge("ViT-g hint", hint, R.encoder_forward(sd, px, heads, bf16_storage=True), R.encoder_forward(sd, px, heads), report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ batch independence, graph
@pytest.mark.parametrize("geom", ["swiglu", "mlp"])
def test_rows_do_not_depend_on_the_batch(geom):
    m, sd, _ = _tiny(geom)
    size = SIZES[geom][1]
    px = T(load_golden(f"dino_tiny_{geom}_out_{size[0]}x{size[1]}")["pixels"]).to(DEV)
    both = m.forward_features(px[:2].contiguous())
    both = [both[k].clone() for k in ("x_prenorm", "x_norm_patchtokens", "x_norm_clstoken")]
    for b in range(2):
        alone = m.forward_features(px[b:b + 1].contiguous())
        for i, k in enumerate(("x_prenorm", "x_norm_patchtokens", "x_norm_clstoken")):
            assert torch.equal(both[i][b:b + 1], alone[k]), f"image {b}, {k}: encoding it with a neighbour changed its rows"


def test_encode_is_capturable_and_allocates_nothing_after_the_first_call():
    e, _ = _tiny_encoder()
    px = T(load_golden("dino_tiny_swiglu_out_42x42")["pixels"])
    static_px = px.to(DEV)
    first = e.encode_pixels(static_px).clone()
    e.encode_pixels(static_px)
    torch.cuda.synchronize()
    before, mem = torch.cuda.memory_stats(DEV)["allocation.all.allocated"], torch.cuda.memory_allocated(DEV)
    for _ in range(10):
        last = e.encode_pixels(static_px)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before, "an encode after the first allocated"
    assert torch.cuda.memory_allocated(DEV) == mem
    assert torch.equal(last, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e.encode_pixels(static_px)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, no side branches: the tower only ever uses the current stream
        out = e.encode_pixels(static_px)
    new_px = px.flip(0).contiguous()
    static_px.copy_(new_px.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    mem = torch.cuda.memory_allocated(DEV)
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == mem
    eager = e.encode_pixels(new_px.to(DEV)).clone()
    assert torch.equal(replayed, eager), "graph replay differs from the eager encode of the same pixels"
    assert not torch.equal(replayed, first)


# ------------------------------------------------------------------------------------------------------------ wiring
def test_control_ldm_conditions_on_the_encoder():
    """ControlLDM at a tiny AnyDoor-shaped geometry (context width = projector_out) whose cond stage is the tiny swiglu encoder:
    get_learned_conditioning(pixels) is [B, 1 + G, projector_out]; one apply_model is finite and differs from the one under unconditional(B)."""
    from anyedit_amd.cldm.cldm import ControlLDM, ControlNet, ControlledUnetModel
    from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder
    from util_models import TINY_UNET
    torch.manual_seed(5)
    gen = torch.Generator().manual_seed(6)
    cfg = dict(TINY_UNET, in_channels=4)
    unet = ControlledUnetModel(**cfg)
    cnet = ControlNet(hint_channels=4, **{k: v for k, v in cfg.items() if k != "out_channels"})
    with torch.no_grad():
        for mod in (unet, cnet):
            for p in mod.parameters():                 # un-zero the zero-initialised layers, or neither the control nor the context reaches the output
                if float(p.abs().sum()) == 0 and p.dim() > 1:
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    sd, _ = _weights("swiglu")
    enc_cfg = {"target": "ldm.modules.encoders.modules.FrozenDinoV2Encoder", "weight": "./not/opened.pth",
               "params": {"config": dict(TINY["swiglu"]), "projector_out": cfg["context_dim"]}}
    model = ControlLDM(cnet, control_key="hint", unet_config=unet, conditioning_key="crossattn", cond_stage_config=enc_cfg, timesteps=1000,
                       linear_start=0.00085, linear_end=0.0120)
    enc = model.cond_stage_model
    assert isinstance(enc, FrozenDinoV2Encoder)
    from anyedit_amd.checkpoints import load_dinov2
    assert load_dinov2(enc, sd) == "dinov2"
    with torch.no_grad():
        enc.projector.weight.copy_(torch.randn(enc.projector.weight.shape, generator=gen) * 0.3)
        enc.projector.bias.copy_(torch.randn(enc.projector.bias.shape, generator=gen) * 0.1)
    model = model.to(DEV).eval()
    B = 2
    px = T(load_golden("dino_tiny_swiglu_out_42x42")["pixels"])[:B].contiguous().to(DEV)
    c = model.get_learned_conditioning(px)
    assert c.shape == (B, 10, cfg["context_dim"]) and c.dtype == BF and torch.isfinite(c.float()).all()
    uc = enc.unconditional(B, size=(42, 42))
    assert uc.shape == c.shape and not torch.equal(uc, c) and torch.equal(c, model.get_learned_conditioning(px))
    x = torch.randn(B, 4, 8, 8, generator=gen).to(DEV)
    hint = torch.randn(B, 4, 64, 64, generator=gen).to(DEV)
    t = torch.tensor([981, 21]).to(DEV)
    eps_c = model.apply_model(x, t, {"c_concat": [hint], "c_crossattn": [c]}).clone()
    eps_u = model.apply_model(x, t, {"c_concat": [hint], "c_crossattn": [uc]}).clone()
    assert eps_c.shape == (B, 4, 8, 8) and torch.isfinite(eps_c).all() and torch.isfinite(eps_u).all()
    assert not torch.equal(eps_c, eps_u), "the reference image must reach the noise prediction"
