"""Host-side checks of the DINOv2 image encoder (no GPU): the chain of trust of its fixtures, the position-table interpolation, the checkpoint
key schema and the three checkpoint forms, the cond-stage wiring, the constructor's and the inputs' refusals, the LayerScale fold and the C ABI's
argument refusals."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import dino_ref as R  # noqa: E402

TINY = {
    "swiglu": dict(embed_dim=128, num_heads=2, depth=2, patch_size=14, img_size=70, mlp_ratio=4.0, ffn_layer="swiglufused"),
    "mlp": dict(embed_dim=192, num_heads=3, depth=2, patch_size=14, img_size=56, mlp_ratio=2.0, ffn_layer="mlp"),
}
SIZES = {"swiglu": [(70, 70), (42, 42), (28, 42)], "mlp": [(56, 56), (84, 84)]}
PROJECTOR_OUT = 96
CASES = [(g, s) for g in TINY for s in SIZES[g]]
CASE_IDS = [f"{g}_{s[0]}x{s[1]}" for g, s in CASES]


def _weights(geom):
    """(tower state dict, encoder state dict or None) of a fixture."""
    arrs = dict(load_golden(f"dino_tiny_{geom}_w0"), **load_golden(f"dino_tiny_{geom}_w1"))
    sd = sub_sd(arrs, "w.")
    proj = sub_sd(arrs, "e.")
    return sd, (dict({"model." + k: v for k, v in sd.items()}, **proj) if proj else None)


def _stored(geom, size):
    return load_golden(f"dino_tiny_{geom}_out_{size[0]}x{size[1]}")


def _tower(geom):
    from anyedit_amd.ldm.modules.encoders.dino_vision import DinoVisionTransformer
    return DinoVisionTransformer(dict(TINY[geom]))


def _encoder(geom="swiglu"):
    from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder
    return FrozenDinoV2Encoder(dict(TINY[geom]), projector_out=PROJECTOR_OUT)


@pytest.mark.parametrize("geom,size", CASES, ids=CASE_IDS)
def test_restatement_matches_the_reference_golden(geom, size):
    """tests/dino_ref.py (fp32) against what the reference's DinoVisionTransformer produced: rel-L2 <= 1e-5 on every stored tensor (the figure
    the CLIP restatements are pinned with; measured at generation: 0 on the tower's outputs — the same torch calls in the same order — and 3e-7
    on the hint, whose normalisation the restatement does in float64)."""
    sd, esd = _weights(geom)
    o = _stored(geom, size)
    cfg = TINY[geom]
    P, C = cfg["patch_size"], cfg["embed_dim"]
    gh, gw = size[0] // P, size[1] // P
    px = T(o["pixels"])
    assert px.shape == (3, 3, *size) and bool((px[2] == 0).all()) and not bool((px[1] == 0).all()) and 0.0 <= float(px.min()) and float(px.max()) <= 1.0
    r = R.dino_forward(sd, px, cfg["num_heads"])
    inter = R.intermediate_layers(r, [0, 1], gh, gw, return_class_token=True)
    got = {"x_norm_clstoken": r["x_norm_clstoken"], "x_norm_patchtokens": r["x_norm_patchtokens"], "x_prenorm": r["x_prenorm"],
           f"pos_interp.{gh}x{gw}": R.pos_table(sd["pos_embed"], gh, gw)}
    for i, (patch, cls) in enumerate(inter):
        got[f"inter.{i}.patch"], got[f"inter.{i}.cls"] = patch, cls
    if esd is not None:
        got["hint"] = R.encoder_forward(esd, px, cfg["num_heads"])
        assert o["hint"].shape == (3, gh * gw + 1, PROJECTOR_OUT)
    assert sorted(got) == sorted(k for k in o if k != "pixels"), "every stored output is checked"
    assert o["x_prenorm"].shape == (3, gh * gw + 1, C) and o["x_norm_patchtokens"].shape == (3, gh * gw, C) and o["x_norm_clstoken"].shape == (3, C)
    assert (o["inter.1.patch"] == o["x_norm_patchtokens"]).all() and (o["inter.1.cls"] == o["x_norm_clstoken"]).all()    # the last block, normed
    worst = 0.0
    for name, v in got.items():
        e = rel_l2(v, T(o[name]))
        worst = max(worst, e)
        assert e <= 1e-5, (geom, size, name, e)
    # the truncated run get_intermediate_layers relies on, and the control: finite, bf16 values, rounding noise and not another function
    r1 = R.dino_forward(sd, px, cfg["num_heads"], n_blocks=1)
    assert len(r1["hidden"]) == 2 and torch.equal(r1["hidden"][1], r["hidden"][1])
    c = R.dino_forward(sd, px, cfg["num_heads"], bf16_storage=True)
    for name in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        assert torch.isfinite(c[name]).all() and torch.equal(c[name], c[name].to(torch.bfloat16).float())
        assert 0 < rel_l2(c[name], T(o[name])) < 5e-2, name
    print(f"{geom} {size}: restatement vs golden: worst rel-L2 {worst:.3e}")


@pytest.mark.parametrize("geom,size", CASES, ids=CASE_IDS)
def test_interpolated_pos_embed_reproduces_the_reference_tables(geom, size):
    """`interpolated_pos_embed` on CPU tensors against the stored output of the reference's interpolate_pos_encoding: the same torch bicubic on
    the same inputs.  BIT EQUALITY held on the machine this was written on (torch CPU, every grid: native 5x5 / 4x4, down 3x3, up 6x6, not
    square 2x3) and is what is asserted."""
    from anyedit_amd.ldm.modules.encoders.dino_vision import interpolated_pos_embed
    sd, _ = _weights(geom)
    o = _stored(geom, size)
    P = TINY[geom]["patch_size"]
    gh, gw = size[0] // P, size[1] // P
    want = T(o[f"pos_interp.{gh}x{gw}"])
    got = interpolated_pos_embed(sd["pos_embed"], gh, gw, 0.1)
    assert got.dtype == torch.float32 and got.shape == (gh * gw + 1, TINY[geom]["embed_dim"]) and got.is_contiguous()
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got, want):.3e}"
    assert torch.equal(got[0], sd["pos_embed"][0, 0]), "the class row is untouched"
    assert torch.equal(interpolated_pos_embed(sd["pos_embed"][0], gh, gw, 0.1), got)           # [1 + N, C] is accepted too
    if gh != gw:                                                                                 # the grid order: rows scale with gh, columns with gw
        assert not torch.equal(interpolated_pos_embed(sd["pos_embed"], gw, gh, 0.1), got)


def test_interpolated_pos_embed_refuses_what_is_not_a_grid():
    from anyedit_amd.ldm.modules.encoders.dino_vision import interpolated_pos_embed
    with pytest.raises(ValueError, match="square grid"):
        interpolated_pos_embed(torch.zeros(1, 7, 8), 2, 2)
    with pytest.raises(ValueError, match="bad grid"):
        interpolated_pos_embed(torch.zeros(1, 5, 8), 0, 2)


def test_key_schema_and_param_count_of_the_default_geometries():
    """ViT-g/14: 40 blocks of 14 tensors + cls / pos / mask tokens + patch conv + norm = 567 tensors named as dinov2_vitg14_pretrain.pth names
    them; 1370 positions (518 / 14 = 37); SwiGLU hidden width 4096; about 1.1 G parameters.  ViT-L / B / S carry fc1 / fc2."""
    from anyedit_amd.ldm.modules.encoders import dino_vision as dv
    assert dv.swiglu_hidden(1536) == 4096 and dv.swiglu_hidden(128) == 344 and dv.swiglu_hidden(384) == 1024
    with torch.device("meta"):
        m = dv.DinoVisionTransformer()
        ml, mb, ms = (dv.DinoVisionTransformer(c) for c in (dv.DINOV2_VITL14, dv.DINOV2_VITB14, dv.DINOV2_VITS14))
        enc = dv.FrozenDinoV2Encoder()
    sd = m.state_dict()
    C, Hd, L = 1536, 4096, 40
    keys = {"cls_token", "pos_embed", "mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias"}
    for i in range(L):
        for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.w12", "mlp.w3"):
            keys |= {f"blocks.{i}.{n}.weight", f"blocks.{i}.{n}.bias"}
        keys |= {f"blocks.{i}.ls1.gamma", f"blocks.{i}.ls2.gamma"}
    assert set(sd) == keys and len(sd) == 7 + 14 * L
    want = 2 * C + 1370 * C + C * 3 * 14 * 14 + C + 2 * C + L * (4 * C + 3 * C * C + 3 * C + C * C + C + 2 * Hd * C + 2 * Hd + C * Hd + C + 2 * C)
    assert sum(v.numel() for v in sd.values()) == want
    assert sd["pos_embed"].shape == (1, 1370, C) and sd["cls_token"].shape == (1, 1, C) and sd["mask_token"].shape == (1, C)
    assert sd["blocks.0.mlp.w12.weight"].shape == (2 * Hd, C) and sd["blocks.39.mlp.w3.weight"].shape == (C, Hd) and sd["patch_embed.proj.weight"].shape == (C, 3, 14, 14)
    assert m.config["layer_norm_eps"] == 1e-6 and m.config["interpolate_offset"] == 0.1 and m.embed_dim == 1536 and m.patch_size == 14
    for tower, (width, depth) in ((ml, (1024, 24)), (mb, (768, 12)), (ms, (384, 12))):
        s = tower.state_dict()
        assert len(s) == 7 + 14 * depth and s[f"blocks.{depth - 1}.mlp.fc1.weight"].shape == (4 * width, width) and "blocks.0.mlp.w12.weight" not in s
    assert set(enc.state_dict()) == {"model." + k for k in keys} | {"projector.weight", "projector.bias"}
    assert enc.state_dict()["projector.weight"].shape == (1024, 1536)
    with torch.device("meta"):                                                                   # init_values None / 0: no LayerScale, no gamma keys
        bare = dv.DinoVisionTransformer(dict(dv.DINOV2_VITS14, init_values=None, depth=1))
    assert not [k for k in bare.state_dict() if "gamma" in k]


@pytest.mark.parametrize("geom", ["swiglu", "mlp"])
def test_fixture_keys_load_strictly(geom):
    sd, esd = _weights(geom)
    m = _tower(geom)
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.state_dict()["blocks.1.ls2.gamma"], sd["blocks.1.ls2.gamma"]) and bool((sd["blocks.1.ls2.gamma"] < 0).any())
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, bogus=torch.zeros(1)))
    if esd is not None:
        e = _encoder(geom)
        assert set(e.state_dict()) == set(esd)
        e.load_state_dict(esd, strict=True)
        assert all(not p.requires_grad for p in e.model.parameters()) and not e.model.training


def test_load_dinov2_accepts_the_three_forms(tmp_path):
    from anyedit_amd.checkpoints import load_dinov2
    torch.manual_seed(0)
    own = {k: torch.randn_like(v) for k, v in _encoder().state_dict().items()}
    bare = {k[len("model."):]: v for k, v in own.items() if k.startswith("model.")}
    anydoor = {"cond_stage_model." + k: v for k, v in own.items()}
    anydoor["model.diffusion_model.out.2.bias"] = torch.zeros(4)                # a neighbour of the prefix in an AnyDoor checkpoint: ignored
    path = tmp_path / "dinov2_tiny_pretrain.pth"
    torch.save(bare, path)
    for form, want in ((bare, "dinov2"), (str(path), "dinov2")):
        tower = _tower("swiglu")
        assert load_dinov2(tower, form) == want
        for k, v in tower.state_dict().items():
            assert torch.equal(v, bare[k]), (want, k)
        enc = _encoder()
        before = enc.projector.weight.detach().clone()
        assert load_dinov2(enc, form) == want
        assert torch.equal(enc.projector.weight, before), "a bare DINOv2 file leaves the projector alone"
        for k, v in enc.model.state_dict().items():
            assert torch.equal(v, bare[k]), (want, k)
    for form, want in ((anydoor, "cond_stage_model"), (own, "encoder")):
        enc = _encoder()
        assert load_dinov2(enc, form) == want
        for k, v in enc.state_dict().items():
            assert torch.equal(v, own[k]), (want, k)
    with pytest.raises(ValueError, match="FrozenDinoV2Encoder"):
        load_dinov2(_tower("swiglu"), own)
    missing = {k: v for k, v in bare.items() if k != "blocks.1.ls1.gamma"}
    with pytest.raises(RuntimeError, match=r"Missing key.*blocks\.1\.ls1\.gamma"):
        load_dinov2(_tower("swiglu"), missing)
    with pytest.raises(RuntimeError, match=r"Missing key.*projector\.bias"):
        load_dinov2(_encoder(), {k: v for k, v in anydoor.items() if not k.endswith("projector.bias")})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        load_dinov2(_tower("swiglu"), dict(bare, **{"register_tokens": torch.zeros(1, 4, 128)}))
    with pytest.raises(RuntimeError, match="Missing key"):                    # a wrong file: the ViT-L layout (fc1 / fc2) into a SwiGLU tower
        load_dinov2(_tower("swiglu"), {k.replace("w12", "fc1").replace("w3", "fc2"): v for k, v in bare.items()})


def test_latent_diffusion_installs_the_encoder(tmp_path):
    from anyedit_amd.cldm.cldm import ControlLDM
    from anyedit_amd.cldm.model import create_model
    from anyedit_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from anyedit_amd.ldm.modules.encoders import modules
    from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder
    from anyedit_amd.ldm.util import get_obj_from_str
    assert modules.FrozenDinoV2Encoder is FrozenDinoV2Encoder                                  # the re-export
    assert get_obj_from_str("ldm.modules.encoders.modules.FrozenDinoV2Encoder") is FrozenDinoV2Encoder
    with pytest.raises(AttributeError):
        modules.FrozenNothing

    class Probe(torch.nn.Module):
        def forward(self, x, t, context=None):
            return x

    built = _encoder()
    m = LatentDiffusion(Probe(), conditioning_key="crossattn", cond_stage_config=built)
    assert m.cond_stage_model is built and not built.training and all(not p.requires_grad for p in built.parameters())
    assert "cond_stage_model.projector.bias" in m.state_dict() and "cond_stage_model.model.blocks.1.mlp.w3.weight" in m.state_dict()
    cfg = {"target": "ldm.modules.encoders.modules.FrozenDinoV2Encoder", "weight": str(tmp_path / "no_such_file.pth"),
           "params": {"config": dict(TINY["swiglu"]), "projector_out": 16}}
    m = LatentDiffusion(Probe(), conditioning_key="crossattn", cond_stage_config=cfg)         # `weight:` accepted and not opened
    assert isinstance(m.cond_stage_model, FrozenDinoV2Encoder) and m.cond_stage_model.projector.weight.shape == (16, 128)
    assert all(not p.requires_grad for p in m.cond_stage_model.parameters())
    called = {}
    m.cond_stage_model.encode = lambda c: called.setdefault("c", c)
    assert m.get_learned_conditioning("pixels") == "pixels"
    # anydoor.yaml's own form: a target and a weight path, no params -> the ViT-g encoder (on the meta device here: 1.1 G parameters)
    with torch.device("meta"):
        probe = LatentDiffusion.__new__(LatentDiffusion)
        torch.nn.Module.__init__(probe)
        probe.instantiate_cond_stage({"target": "ldm.modules.encoders.modules.FrozenDinoV2Encoder",
                                      "weight": "./checkpoints/visual_models/anydoor/checkpoints/dinov2_vitg14_pretrain.pth"})
    assert isinstance(probe.cond_stage_model, FrozenDinoV2Encoder) and probe.cond_stage_model.projector.weight.shape == (1024, 1536)
    assert len(probe.cond_stage_model.model.blocks) == 40
    # a ControlLDM from a YAML in anydoor.yaml's shape (tiny widths): its cond stage is the encoder
    tiny = "image_size: 8\n        in_channels: 4\n        model_channels: 32\n        attention_resolutions: [1, 2]\n        " \
           "num_res_blocks: 1\n        channel_mult: [1, 2]\n        num_head_channels: 8\n        use_spatial_transformer: true\n        " \
           "use_linear_in_transformer: true\n        transformer_depth: 1\n        context_dim: 16\n        legacy: false\n"
    yaml_text = f"""model:
  target: AnyEdit_Collection.other_modules.cldm.cldm.ControlLDM
  params:
    linear_start: 0.00085
    linear_end: 0.0120
    timesteps: 1000
    image_size: 8
    channels: 4
    cond_stage_key: ref
    cond_stage_trainable: false
    conditioning_key: crossattn
    scale_factor: 0.18215
    use_ema: false
    only_mid_control: false
    control_key: hint
    control_stage_config:
      target: AnyEdit_Collection.other_modules.cldm.cldm.ControlNet
      params:
        hint_channels: 4
        {tiny}
    unet_config:
      target: AnyEdit_Collection.other_modules.cldm.cldm.ControlledUnetModel
      params:
        out_channels: 4
        {tiny}
    cond_stage_config:
      target: ldm.modules.encoders.modules.FrozenDinoV2Encoder
      weight: ./checkpoints/visual_models/anydoor/checkpoints/dinov2_vitg14_pretrain.pth
      params:
        projector_out: 16
        config: {{embed_dim: 128, num_heads: 2, depth: 2, img_size: 70, ffn_layer: swiglufused}}
"""
    path = tmp_path / "tiny_anydoor.yaml"
    path.write_text(yaml_text)
    model = create_model(str(path))
    assert isinstance(model, ControlLDM) and isinstance(model.cond_stage_model, FrozenDinoV2Encoder)
    assert len([k for k in model.state_dict() if k.startswith("cond_stage_model.model.")]) == 7 + 14 * 2
    with pytest.raises(ValueError, match="GPU only"):                                            # reaches the tower, which has no CPU path
        model.get_learned_conditioning(torch.zeros(1, 3, 28, 28))


def test_geometry_outside_the_kernels_is_refused_at_construction():
    from anyedit_amd.ldm.modules.encoders.dino_vision import DinoVisionTransformer, FrozenDinoV2Encoder
    base = TINY["swiglu"]
    with torch.device("meta"):
        for bad, msg in ((dict(num_register_tokens=4), "register tokens"), (dict(interpolate_antialias=True), "interpolate_antialias"),
                         (dict(ffn_layer="identity"), "identity"), (dict(ffn_layer="moe"), "ffn_layer"),
                         (dict(embed_dim=208, num_heads=2), "head_dim"),            # 104: ViT-bigG's
                         (dict(embed_dim=100, num_heads=1), "multiple of 8"), (dict(embed_dim=2560, num_heads=40), "at most 2048"),
                         (dict(img_size=72), "img_size")):
            with pytest.raises(ValueError, match=msg):
                DinoVisionTransformer(dict(base, **bad))
        with pytest.raises(ValueError, match="projector_out"):
            FrozenDinoV2Encoder(dict(base), projector_out=30)


def test_input_refusals_need_no_gpu():
    m = _tower("swiglu")
    e = _encoder()
    ok = torch.zeros(1, 3, 28, 42)
    with pytest.raises(ValueError, match="masks"):
        m.forward_features(ok, masks=torch.zeros(1, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="masks"):
        m(ok, masks=torch.zeros(1, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="GPU only"):
        m.forward_features(ok)
    with pytest.raises(ValueError, match="GPU only"):
        e.encode([ok, ok])
    with pytest.raises(ValueError, match="whole number"):
        m(torch.zeros(1, 3, 30, 28))
    with pytest.raises(ValueError, match="whole number"):
        m(torch.zeros(1, 3, 0, 28))
    with pytest.raises(TypeError, match="fp32"):
        m(torch.zeros(1, 3, 28, 28, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one size"):
        m([ok, torch.zeros(1, 3, 28, 28)])
    with pytest.raises(ValueError, match="one size"):
        m(torch.zeros(1, 4, 28, 28))
    with pytest.raises(ValueError, match="empty list"):
        m([])
    with pytest.raises(ValueError, match="outside"):
        m.get_intermediate_layers(ok, n=[2])
    with pytest.raises(ValueError, match="outside"):
        m.get_intermediate_layers(ok, n=3)
    assert m._ws == {} and e.model._ws == {}                                  # refused before a workspace existed


def test_layerscale_is_folded_in_fp32_and_follows_the_parameters():
    """`packed()` holds round_bf16(gamma[:, None] * W) and gamma * b for attn.proj and mlp.w3 / mlp.fc2, nothing else scaled; an in-place change
    of a gamma rebuilds the fold."""
    bf = lambda t: t.to(torch.bfloat16)
    for geom, last in (("swiglu", "w3"), ("mlp", "fc2")):
        sd, _ = _weights(geom)
        m = _tower(geom)
        m.load_state_dict(sd)
        blk = m.blocks[1]
        p = blk.packed()
        assert blk.packed() is p
        q = "blocks.1."
        g1, g2 = sd[q + "ls1.gamma"], sd[q + "ls2.gamma"]
        assert torch.equal(p.wo, bf(g1[:, None] * sd[q + "attn.proj.weight"])) and torch.equal(p.bo, g1 * sd[q + "attn.proj.bias"])
        assert torch.equal(p.w2, bf(g2[:, None] * sd[q + f"mlp.{last}.weight"])) and torch.equal(p.b2, g2 * sd[q + f"mlp.{last}.bias"])
        assert not torch.equal(p.wo, bf(sd[q + "attn.proj.weight"]))
        assert torch.equal(p.wqkv, bf(sd[q + "attn.qkv.weight"])) and p.bo.dtype == torch.float32 and p.wo.dtype == torch.bfloat16
        first = "w12" if geom == "swiglu" else "fc1"
        assert torch.equal(p.w1, bf(sd[q + f"mlp.{first}.weight"])) and torch.equal(p.b1, sd[q + f"mlp.{first}.bias"])
        tok = m.weights_token()
        with torch.no_grad():
            blk.ls2.gamma.mul_(2.0)
        p2 = blk.packed()
        assert p2 is not p and torch.equal(p2.w2, bf(2.0 * g2[:, None] * sd[q + f"mlp.{last}.weight"])) and torch.equal(p2.wo, p.wo)
        assert m.weights_token() != tok
    t = m._tables()
    assert m._tables() is t and t.wpatch.shape == (192, 640) and t.cls.shape == (192,) and t.bpatch.dtype == torch.float32
    assert torch.allclose(t.mean, torch.tensor(R.IMAGENET_MEAN)) and torch.allclose(t.std, torch.tensor(R.IMAGENET_STD))
    # the position table is cached per grid against pos_embed
    a = m.pos_table(6, 6)
    assert m.pos_table(6, 6) is a and a.shape == (37, 192) and m.pos_table(4, 4).shape == (17, 192)
    with torch.no_grad():
        m.pos_embed.add_(1.0)
    assert m.pos_table(6, 6) is not a and torch.allclose(m.pos_table(6, 6), a + 1.0, atol=1e-5)


def test_library_exports_the_new_symbols_and_refuses_bad_arguments():
    from anyedit_amd import _lib
    L = _lib.lib
    for name in ("ae_dino_embed_bf16", "ae_swiglu_f32_bf16"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    buf = (ctypes.c_uint16 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15                    # host memory: every call below must be refused before it is touched
    e = L.ae_dino_embed_bf16
    for args in ((None, 128, p, p, p, p), (p, 128, None, p, p, p), (p, 128, p, None, p, p), (p, 128, p, p, None, p), (p, 128, p, p, p, None)):
        assert e(*args, 1, 4, 128, None) == -1 and b"null pointer" in L.ae_last_error()
    assert e(p, 100, p, p, p, p, 1, 4, 100, None) == -1 and b"multiple of 8" in L.ae_last_error()
    assert e(p, 128, p, p, p, p, 0, 4, 128, None) == -1 and b"bad sizes" in L.ae_last_error()
    assert e(p, 128, p, p, p, p, 1, 0, 128, None) == -1 and b"bad sizes" in L.ae_last_error()
    assert e(p, 128, p, p, p, p, 1, 4, -8, None) == -1 and b"bad sizes" in L.ae_last_error()
    assert e(p, 64, p, p, p, p, 1, 4, 128, None) == -1 and b"row stride" in L.ae_last_error()
    assert e(p, 130, p, p, p, p, 1, 4, 128, None) == -1 and b"row stride" in L.ae_last_error()
    assert e(p, 128, p, p, p + 8, p, 1, 4, 128, None) == -1 and b"aligned" in L.ae_last_error()
    s = L.ae_swiglu_f32_bf16
    for args in ((None, 688, p, p), (p, 688, None, p), (p, 688, p, None)):
        assert s(*args, 344, 4, 344, None) == -1 and b"null pointer" in L.ae_last_error()
    assert s(p, 688, p, p, 344, 4, 340, None) == -1 and b"multiple of 8" in L.ae_last_error()
    assert s(p, 688, p, p, 344, 0, 344, None) == -1 and b"bad sizes" in L.ae_last_error()
    assert s(p, 688, p, p, 344, 4, 0, None) == -1 and b"bad sizes" in L.ae_last_error()
    assert s(p, 688, p, p, 344, -1, 344, None) == -1 and b"bad sizes" in L.ae_last_error()
    assert s(p, 680, p, p, 344, 4, 344, None) == -1 and b"u row stride" in L.ae_last_error()
    assert s(p, 690, p, p, 344, 4, 344, None) == -1 and b"u row stride" in L.ae_last_error()
    assert s(p, 688, p, p, 336, 4, 344, None) == -1 and b"y row stride" in L.ae_last_error()
    assert s(p, 688, p, p, 348, 4, 344, None) == -1 and b"y row stride" in L.ae_last_error()
    assert s(p, 688, p + 4, p, 344, 4, 344, None) == -1 and b"aligned" in L.ae_last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    from anyedit_amd import ops
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.dino_embed(torch.zeros(4, 8), torch.zeros(8), torch.zeros(8), torch.zeros(5, 8), 1)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.swiglu(torch.zeros(4, 16), torch.zeros(16))
