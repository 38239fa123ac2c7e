"""GPU tests of the CLIP vision tower: its three kernels against float64 between sentinel guards, the attention route it depends on at its
own shapes, both tiny towers against the transformers golden and the full-width towers against the restatement (under the project's
1.5 x control rule), batch independence, graph capture without allocations, and the MoE / pipeline / trainer wiring.  Every case runs once."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import clip_vision_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0x7FA5          # a NaN bit pattern no kernel writes
GUARD = 4096
TINY = {
    "quick_gelu": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=70,
                       projection_dim=96, hidden_act="quick_gelu", layer_norm_eps=1e-5),
    "gelu": dict(hidden_size=160, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=16, image_size=48,
                 projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5),
}
STORED = ["image_embeds", "last_hidden_state", "pooler_output", "hidden_states.0", "hidden_states.1", "hidden_states.2"]


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


# ------------------------------------------------------------------------------------------------------------ patch rows
@pytest.mark.parametrize("dtype", [torch.float32, BF, torch.uint8], ids=["fp32", "bf16", "uint8"])
@pytest.mark.parametrize("shape", [(2, 28, 42, 14), (1, 32, 32, 16), (3, 64, 64, 32)], ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}_P{s[3]}")
def test_patch_rows_vs_unfold_and_float64(shape, dtype):
    """Normalisation off: exactly torch's unfold of the input, rounded to bf16.  On: every element within one bf16 step (2^-8 |ref|) of the
    float64 formula (x * rescale - mean[c]) / std[c].  Pad columns are zeros although the buffer held the NaN sentinel."""
    from anyedit_amd import ops
    B, H, W, P = shape
    gen = torch.Generator().manual_seed(H * 100 + P + B)
    if dtype == torch.uint8:
        x = torch.randint(0, 256, (B, 3, H, W), generator=gen, dtype=torch.uint8)
        rescale = 1.0 / 255.0
    else:
        x = torch.randn(B, 3, H, W, generator=gen).to(dtype)
        rescale = 0.75
    K, Kpad = 3 * P * P, ops.clip_patch_kpad(3, P)
    M = B * (H // P) * (W // P)
    xd = x.to(DEV)
    unfold = lambda t: F.unfold(t, P, stride=P).transpose(1, 2).reshape(M, K)       # column c P^2 + ky P + kx of row (b, gy, gx)
    plain = _twice((M, Kpad), lambda out: ops.clip_patch_rows(xd, P, out=out))
    assert torch.equal(plain[:, :K], unfold(x.float()).to(BF)), "plain conversion must equal unfold exactly"
    assert bool((plain[:, K:].view(torch.int16) == 0).all()), "pad columns must be written as zeros"
    mean, std = torch.tensor(R.OPENAI_CLIP_MEAN), torch.tensor(R.OPENAI_CLIP_STD)
    got = _twice((M, Kpad), lambda out: ops.clip_patch_rows(xd, P, rescale, mean.to(DEV), std.to(DEV), out=out))
    r32 = float(torch.tensor(rescale, dtype=torch.float32))
    ref = unfold((x.to(F64) * r32 - mean.to(F64).view(1, 3, 1, 1)) / std.to(F64).view(1, 3, 1, 1))
    err = (got[:, :K].to(F64) - ref).abs()
    ratio = float((err / (2.0 ** -8 * ref.abs() + 1e-30)).max())
    print(f"patch rows {shape} {dtype}: worst |err| / (2^-8 |ref|) = {ratio:.3f}")
    assert ratio <= 1.0
    assert bool((got[:, K:].view(torch.int16) == 0).all()), "pad columns must be written as zeros"


# ------------------------------------------------------------------------------------------------------------ embed + LayerNorm, pooled LayerNorm
def _ln64(x, gamma, beta, eps):
    x = x.to(F64)
    xh = (x - x.mean(-1, keepdim=True)) / (x.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    ref = xh * gamma.to(F64) + beta.to(F64)
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ((xh * gamma.to(F64)).abs() + beta.to(F64).abs()) + 1e-30


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", [1, 9, 256])
@pytest.mark.parametrize("C", [8, 128, 1280, 1664])
def test_embed_ln_vs_float64(C, G, B):
    """Every element within 2^-8 |ref| + 2^-16 (|gamma x^| + |beta|) of float64 (one bf16 rounding + fp32 statistics); the class row is the
    same bits in every sample."""
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(C * 1000 + G * 10 + B)
    patch = torch.randn(B * G, C, generator=gen) * 0.7
    cls, pos = torch.randn(C, generator=gen) * 0.3, torch.randn(G + 1, C, generator=gen) * 0.3
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    d = [t.to(DEV) for t in (patch, cls, pos, gamma, beta)]
    N = G + 1
    got = _twice((B * N, C), lambda out: ops.clip_vision_embed_ln(d[0], d[1], d[2], d[3], d[4], 1e-5, B, out=out)).view(B, N, C)
    x = torch.cat([cls.to(F64).expand(B, 1, C), patch.to(F64).view(B, G, C)], 1) + pos.to(F64)
    ref, bnd = _ln64(x, gamma, beta, 1e-5)
    ratio = float(((got.to(F64) - ref).abs() / bnd).max())
    print(f"embed + LN C={C} G={G} B={B}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    for b in range(1, B):
        assert torch.equal(got[b, 0], got[0, 0]), "the class row must not depend on the sample"


@pytest.mark.parametrize("BN", [(1, 1), (3, 10), (5, 257)], ids=lambda v: f"B{v[0]}_N{v[1]}")
@pytest.mark.parametrize("C", [8, 128, 1280, 1664])
def test_pool_ln_reads_only_the_class_rows(C, BN):
    """Rows b N picked by stride out of a buffer whose other rows hold the NaN sentinel; same bound as embed + LN."""
    from anyedit_amd import ops
    B, N = BN
    gen = torch.Generator().manual_seed(C * 100 + N)
    rows = torch.randn(B, C, generator=gen).to(BF)
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    x = torch.empty(B * N, C, dtype=BF, device=DEV)
    x.view(torch.int16).fill_(SENT)
    x[::N] = rows.to(DEV)
    g, e = gamma.to(DEV), beta.to(DEV)
    got = _twice((B, C), lambda out: ops.clip_vision_pool_ln(x, N, g, e, 1e-5, out=out))
    ref, bnd = _ln64(rows, gamma, beta, 1e-5)
    ratio = float(((got.to(F64) - ref).abs() / bnd).max())
    print(f"pool LN C={C} B={B} N={N}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from anyedit_amd import ops, _lib
    with pytest.raises(_lib.AnyEditHipError, match="> 2048"):
        ops.clip_vision_pool_ln(torch.zeros(2, 2056, dtype=BF, device=DEV), 1, torch.ones(2056, device=DEV), torch.zeros(2056, device=DEV), 1e-5)
    with pytest.raises(ValueError, match="whole number"):
        ops.clip_patch_rows(torch.zeros(1, 3, 30, 28, device=DEV), 14)
    with pytest.raises(TypeError, match="contiguous"):
        ops.clip_patch_rows(torch.zeros(1, 3, 28, 56, device=DEV)[..., ::2], 14)


# ------------------------------------------------------------------------------------------------------------ the attention route the tower uses
@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("N", [10, 26, 50, 197, 257])
def test_attention_at_the_towers_shapes(N, D):
    """The attention launch of the tower (`clip_vision.attention_rows`: `ops.attention` / ae_attn_fwd_bf16 on packed q | k | v rows with the tower's
    strides), every element against float64 under the bound tools/route_check.py applies to attention: |got - ref| <= 2^-8 |ref| +
    2^-8 (P @ |V|).  A guard of the route the tower depends on: attention.hip at D = 64; at D = 80 attention_fast.hip from 64 tokens up and,
    through the all-ones key mask `attention_rows` passes below that, the general kernel of attention.hip.

    Why the mask: on one MI355X the unmasked call measured, worst |err| / bound, D = 64: 0.586 / 0.545 / 0.412 / 0.336 / 0.320 at N = 10 / 26 / 50 /
    197 / 257; D = 80 (attention_fast.hip): 1.0014 / 0.789 / 0.661 / 0.537 / 0.509 — N = 10 missed the bound.  attention_fast.hip rounds
    Q * scale * log2(e) to bf16 before the logit MFMA, an error the bound has no term for and one that weighs most where few keys share the
    probability mass; the tower is routed around it below one 64-key tile ("Finding")."""
    from anyedit_amd.ldm.modules.encoders.clip_vision import attention_rows
    B, H = 2, 2
    C = H * D
    gen = torch.Generator().manual_seed(1000 * N + D)
    qkv = torch.randn(B * N, 3 * C, generator=gen).to(BF)
    dq = qkv.to(DEV)
    got = _twice((B * N, C), lambda out: attention_rows(dq, B, H, N, D, out))
    got = got.to(F64).view(B, N, H, D).transpose(1, 2)
    x = qkv.to(F64).view(B, N, 3, H, D)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    P = ((q @ k.transpose(-1, -2)) * D ** -0.5).softmax(-1)
    ref = P @ v
    bnd = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * (P @ v.abs()) + 1e-30
    ratio = float(((got - ref).abs() / bnd).max())
    print(f"attention N={N} D={D}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ tiny towers vs golden
def _tiny(act):
    from anyedit_amd.ldm.modules.encoders.clip_vision import CLIPVisionModelWithProjection
    sd = sub_sd(load_golden("clip_vision_tiny_" + act), "w.")
    m = CLIPVisionModelWithProjection(dict(TINY[act]))
    m.load_state_dict(sd)
    return m.to(DEV).eval().requires_grad_(False), sd, load_golden(f"clip_vision_tiny_{act}_out")


def _pick(r, name):
    return r["hidden_states"][int(name.split(".")[1])] if name.startswith("hidden_states.") else r[name]


def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_tiny_tower_vs_transformers_golden(act):
    """Every stored output of the fixture (the all-zero image is in its batch): err(HIP) <= 1.5 x err(control), control =
    clip_vision_ref(bf16_storage=True) on the same weights; through forward(output_hidden_states=True) and through encode_pixels(layer) for
    every valid layer."""
    m, sd, o = _tiny(act)
    cfg = TINY[act]
    L, heads = cfg["num_hidden_layers"], cfg["num_attention_heads"]
    px = T(o["pixel_values"])
    assert bool((px[2] == 0).all())
    ctl = R.clip_vision_forward(sd, px, heads, act=act, bf16_storage=True)
    report, ok = [], True
    pd = px.to(DEV)
    out = m(pd, output_hidden_states=True)
    N = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    assert out.image_embeds.shape == (3, cfg["projection_dim"]) and out.last_hidden_state.shape == (3, N, cfg["hidden_size"]) and len(out.hidden_states) == L + 1
    assert out[0] is out.image_embeds and out[1] is out.last_hidden_state and out[2] is out.hidden_states
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1])               # no final norm
    mine = dict(image_embeds=out.image_embeds, last_hidden_state=out.last_hidden_state, pooler_output=out.pooler_output, hidden_states=out.hidden_states)
    for name in STORED:
        ok &= _judge("forward()." + name, _pick(mine, name), _pick(ctl, name), T(o[name]), report)
    assert m(pd).hidden_states is None
    for layer in list(range(L + 1)) + [-1, -2, -3]:
        h = m.encode_pixels(pd, layer)
        assert h.shape == (3, N, cfg["hidden_size"]) and h.dtype == BF
        ok &= _judge(f"encode_pixels(layer={layer})", h, ctl["hidden_states"][layer], T(o[f"hidden_states.{layer % (L + 1)}"]), report)
    print("\n".join(report))
    assert ok, "\n".join(report)


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_uint8_pixels_equal_host_normalised_pixels_within_the_rule(act):
    """Raw uint8 pixels through the fused rescale + normalise against the restatement on the same pixels normalised on the host."""
    m, sd, o = _tiny(act)
    cfg = TINY[act]
    u8 = T(o["pixels_u8"])
    host = R.normalize_u8(u8)
    ref = R.clip_vision_forward(sd, host, cfg["num_attention_heads"], act=act)
    ctl = R.clip_vision_forward(sd, host, cfg["num_attention_heads"], act=act, bf16_storage=True)
    report, ok = [], True
    out = m(u8.to(DEV), output_hidden_states=True)
    ok &= _judge("uint8 image_embeds", out.image_embeds, ctl["image_embeds"], ref["image_embeds"], report)
    for i in range(3):
        ok &= _judge(f"uint8 hidden_states[{i}]", out.hidden_states[i], ctl["hidden_states"][i], ref["hidden_states"][i], report)
    ok &= _judge("uint8 encode_pixels(-2)", m.encode_pixels(u8.to(DEV)), ctl["hidden_states"][-2], ref["hidden_states"][-2], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ full width, two layers
@pytest.mark.parametrize("name", ["ViT-H", "ViT-L"])
def test_full_width_tower_vs_restatement(name):
    """The real geometry (224 px, 257 tokens, B = 2) cut to two layers, seeded weights: hidden_states[0..2] and image_embeds under the
    1.5 x control rule.  Two layers carry every shape of the real tower at a sixteenth of the CPU cost."""
    from anyedit_amd.ldm.modules.encoders import clip_vision as cv
    cfg = dict(cv.CLIP_VIT_H_14_VISION if name == "ViT-H" else cv.CLIP_VIT_L_14_VISION, num_hidden_layers=2)
    sd = R.seeded_state_dict(cfg, seed=0)
    with torch.device("meta"):
        m = cv.CLIPVisionModelWithProjection(cfg)
    m.load_state_dict(sd, assign=True)
    m = m.to(DEV)
    px = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    heads, act = cfg["num_attention_heads"], cfg["hidden_act"]
    ref = R.clip_vision_forward(sd, px, heads, act=act)
    ctl = R.clip_vision_forward(sd, px, heads, act=act, bf16_storage=True)
    out = m(px.to(DEV), output_hidden_states=True)
    assert out.hidden_states[0].shape == (2, 257, cfg["hidden_size"])
    report, ok = [], True
    for i in range(3):
        ok &= _judge(f"{name} hidden_states[{i}]", out.hidden_states[i], ctl["hidden_states"][i], ref["hidden_states"][i], report)
    ok &= _judge(f"{name} image_embeds", out.image_embeds, ctl["image_embeds"], ref["image_embeds"], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ batch independence, graph
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_rows_do_not_depend_on_the_batch(act):
    m, sd, o = _tiny(act)
    px = T(o["pixel_values"]).to(DEV)
    both = m(px[:2].contiguous(), output_hidden_states=True)
    both = [h.clone() for h in both.hidden_states] + [both.image_embeds.clone()]
    for b in range(2):
        alone = m(px[b:b + 1].contiguous(), output_hidden_states=True)
        for i, (x, y) in enumerate(zip(both, list(alone.hidden_states) + [alone.image_embeds])):
            assert torch.equal(x[b:b + 1], y), f"image {b}, output {i}: encoding it with a neighbour changed its rows"


def test_encode_is_capturable_and_allocates_nothing_after_the_first_call():
    m, sd, o = _tiny("quick_gelu")
    px = T(o["pixel_values"])
    static_px = px.to(DEV)
    first = m.encode_pixels(static_px).clone()
    m.encode_pixels(static_px)
    torch.cuda.synchronize()
    before, mem = torch.cuda.memory_stats(DEV)["allocation.all.allocated"], torch.cuda.memory_allocated(DEV)
    for _ in range(10):
        last = m.encode_pixels(static_px)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before, "an encode after the first allocated"
    assert torch.cuda.memory_allocated(DEV) == mem
    assert torch.equal(last, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.encode_pixels(static_px)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, no side branches: the tower only ever uses the current stream
        out = m.encode_pixels(static_px)
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
    eager = m.encode_pixels(new_px.to(DEV)).clone()
    assert torch.equal(replayed, eager), "graph replay differs from the eager encode of the same pixels"
    assert not torch.equal(replayed, first)


# ------------------------------------------------------------------------------------------------------------ wiring
def _tiny_moe(seed, tower):
    from util_models import TINY_UNET, unzero, randomize_norm_affine, G
    from anyedit_amd.anysd.model import MoE
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    torch.manual_seed(seed)
    unet = UNetModel(**dict(TINY_UNET, context_dim=64))
    unzero(unet, G(seed), std=0.05)
    randomize_norm_affine(unet, G(seed + 1))
    return MoE(unet.eval(), image_encoder=tower, expert_num=11, n_tasks=6, context_dim=64, clip_dim=128, ip_tokens=4)


def test_moe_and_pipeline_take_reference_images():
    from anyedit_amd.anysd.model import MoE
    from anyedit_amd.anysd.pipeline import EditPipeline
    from anyedit_amd.ldm.models.diffusion.ddpm import DDPM
    tower, sd, o = _tiny("quick_gelu")
    with pytest.raises(ValueError, match="clip_dim"):
        MoE(_tiny_moe(7, None).unet, image_encoder=tower, clip_dim=32, context_dim=64)
    moe = _tiny_moe(7, tower).eval().requires_grad_(False).to(DEV)
    gen = torch.Generator().manual_seed(9)
    B = 2
    px = T(o["pixel_values"])[:B].contiguous().to(DEV)
    emb = moe.reference_embeds(px)
    assert emb.shape == (B, 26, 128) and emb.dtype == BF
    assert torch.equal(emb, tower.encode_pixels(px, -2)) and emb.data_ptr() != tower.encode_pixels(px, -2).data_ptr()     # a copy the caller owns
    x = torch.randn(B, 8, 8, 8, generator=gen).to(DEV)
    t = torch.tensor([981, 21]).to(DEV)
    ehs = torch.randn(B, 77, 64, generator=gen).to(DEV)
    code = torch.tensor([1, 3]).to(DEV)
    with torch.no_grad():
        from_px = moe(x, t, ehs, px, code).clone()
        from_emb = moe(x, t, ehs, emb, code).clone()
    assert torch.isfinite(from_px).all() and torch.equal(from_px, from_emb), "MoE.forward on pixel values must equal forward on reference_embeds(pixels)"

    sched = DDPM(moe.unet, timesteps=1000, linear_start=0.00085, linear_end=0.0120).to(DEV)
    x_T = torch.randn(B, 4, 8, 8, generator=gen).to(DEV)
    img_lat = (torch.randn(B, 4, 8, 8, generator=gen) * 0.18215).to(DEV)
    null = torch.randn(1, 77, 64, generator=gen).to(DEV)
    pipe = EditPipeline(moe, sched, use_graph=True)
    from_images = pipe.edit(x_T, img_lat, ehs, null, None, code, steps=4, reference_images=px).clone()
    plain = pipe.edit(x_T, img_lat, ehs, null, emb, code, steps=4).clone()
    assert torch.isfinite(plain).all() and torch.equal(from_images, plain), "edit(reference_images=) must equal edit on the pre-computed embeddings, bit for bit"
    other = pipe.edit(x_T, img_lat, ehs, null, None, code, steps=4, reference_images=px.flip(0).contiguous())
    assert not torch.equal(other, plain), "changing the reference image must change the latents"
    with pytest.raises(ValueError, match="not both"):
        pipe.edit(x_T, img_lat, ehs, null, emb, code, steps=4, reference_images=px)
    bare = EditPipeline(_tiny_moe(7, None).eval().requires_grad_(False).to(DEV), sched, use_graph=False)
    with pytest.raises(ValueError, match="image_encoder"):
        bare.edit(x_T, img_lat, ehs, null, None, code, steps=4, reference_images=px)


def test_edit_text_takes_reference_images():
    from anyedit_amd.anysd.pipeline import EditPipeline
    from anyedit_amd.ldm.models.diffusion.ddpm import DDPM
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    import clip_ref
    tower, sd, o = _tiny("quick_gelu")
    moe = _tiny_moe(17, tower).eval().requires_grad_(False).to(DEV)
    cfg = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
               eos_token_id=255, pad_token_id=255, bos_token_id=254)
    te = FrozenCLIPEmbedder(config=cfg)
    te.load_state_dict(clip_ref.seeded_state_dict(cfg, seed=3))
    te = te.to(DEV)
    sched = DDPM(moe.unet, timesteps=1000, linear_start=0.00085, linear_end=0.0120).to(DEV)
    gen = torch.Generator().manual_seed(19)
    B = 2
    x_T = torch.randn(B, 4, 8, 8, generator=gen).to(DEV)
    img_lat = (torch.randn(B, 4, 8, 8, generator=gen) * 0.18215).to(DEV)
    ids = torch.randint(0, 250, (B, 77), generator=gen)
    ids[:, 0], ids[0, 12:], ids[1, 40:] = 254, 255, 255
    code = torch.tensor([1, 3]).to(DEV)
    px = T(o["pixel_values"])[:B].contiguous().to(DEV)
    pipe = EditPipeline(moe, sched, use_graph=True, text_encoder=te)
    a = pipe.edit_text(x_T, img_lat, ids, None, code, reference_images=px, steps=4).clone()
    b = pipe.edit_text(x_T, img_lat, ids, moe.reference_embeds(px), code, steps=4).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_trainer_takes_reference_clip_images():
    """train.py:683-691: a batch may carry reference_clip_images; the loss equals the one from their penultimate hidden states, bit for bit."""
    from anyedit_amd.anysd.train import AnySDTrainer
    from oracle import schedule_ref as S
    tower, sd, o = _tiny("quick_gelu")
    moe = _tiny_moe(11, tower).to(DEV)
    buffers = S.register_schedule("linear", 1000, 0.00085, 0.0120)
    sa, s1 = (torch.as_tensor(np.asarray(buffers[k])).float().to(DEV) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))
    gen = torch.Generator().manual_seed(13)
    B = 2
    lat, img, noise = (torch.randn(B, 4, 8, 8, generator=gen).to(DEV) for _ in range(3))
    ehs = torch.randn(B, 77, 64, generator=gen).to(DEV)
    code, t = torch.tensor([1, 3]).to(DEV), torch.tensor([981, 21]).to(DEV)
    px = T(o["pixel_values"])[1:3].contiguous().to(DEV)                            # one real image, one all-zero reference (train.py:682)
    tr = AnySDTrainer(moe, sa, s1)
    assert not any(k.startswith("image_encoder") for k in tr.params)               # the tower is frozen
    loss_px, _, _ = tr.forward_loss(lat, img, ehs, px, code, noise, t)
    loss_emb, _, _ = tr.forward_loss(lat, img, ehs, moe.reference_embeds(px), code, noise, t)
    assert torch.isfinite(loss_px).all() and torch.equal(loss_px, loss_emb)
    with pytest.raises(ValueError, match="image_encoder"):
        AnySDTrainer(_tiny_moe(11, None).to(DEV), sa, s1).forward_loss(lat, img, ehs, px, code, noise, t)
