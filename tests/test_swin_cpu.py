"""Host-side checks of GroundingDINO's Swin backbone (no GPU): the chain of trust of its fixtures, the relative position index, the kernel's
closed forms for the shift mask and the row addressing against the reference-style constructions, the checkpoint key schema and the three
checkpoint forms, the constructor's refusals and the C ABI's exports and argument refusals."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, rel_l2, T  # noqa: E402
import swin_ref as R  # noqa: E402

TINY = {
    "a": dict(embed_dim=32, depths=[2, 2, 2], num_heads=[1, 2, 4], window_size=7),
    "b": dict(embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=12),
}
SIZES = {"a": [(50, 38)], "b": [(90, 106), (40, 40)]}
CASES = [(g, s) for g in TINY for s in SIZES[g]]
CASE_IDS = [f"{g}_{s[0]}x{s[1]}" for g, s in CASES]


def weights(geom):
    arrs = {}
    for i in range(len(TINY[geom]["depths"])):
        arrs.update(load_golden(f"swin_tiny_{geom}_w{i}"))
    return R.fixture_state_dict(arrs)


def stored(geom, size):
    return load_golden(f"swin_tiny_{geom}_out_{size[0]}x{size[1]}")


def tower(geom, **kw):
    from anyedit_amd.groundingdino.swin_transformer import SwinTransformer
    cfg = TINY[geom]
    return SwinTransformer(out_indices=tuple(range(len(cfg["depths"]))), **cfg, **kw)


def stage_maps(geom, size):
    """(H, W) of the token map of every stage."""
    h, w = (size[0] + 3) // 4, (size[1] + 3) // 4
    out = []
    for _ in TINY[geom]["depths"]:
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


@pytest.mark.parametrize("geom,size", CASES, ids=CASE_IDS)
def test_restatement_matches_the_reference_golden(geom, size):
    """tests/swin_ref.py (fp32) against what the reference's SwinTransformer produced: rel-L2 <= 1e-5 on every stored output (the figure the
    DINOv2 restatement is pinned with; measured at generation: 0 — the same torch calls in the same order)."""
    sd, o, cfg = weights(geom), stored(geom, size), TINY[geom]
    px = T(o["pixels"])
    assert px.shape == (2, 3, *size)
    r = R.swin_forward(sd, px, cfg)
    got = {f"out.{i}": t for i, t in enumerate(r["outs"])}
    got["stage1_in"] = r["stage_in"][1]
    if "mask_in" in o:
        m = T(o["mask_in"])
        assert m.dtype == torch.bool and bool(m.any()) and not bool(m.all())
        for i, mk in enumerate(R.nested_masks(m, [t.shape[-2:] for t in r["outs"]])):
            assert torch.equal(mk, T(o[f"mask.{i}"])), (geom, size, i)
            assert bool(mk.any()) and not bool(mk.all())
    assert sorted(got) == sorted(k for k in o if k.startswith(("out.", "stage1_in"))), "every stored output is checked"
    for (h, w), i in zip(stage_maps(geom, size), range(len(cfg["depths"]))):
        assert o[f"out.{i}"].shape == (2, cfg["embed_dim"] * 2 ** i, h, w)
    for name, v in got.items():
        e = rel_l2(v, T(o[name]))
        assert e <= 1e-5, (geom, size, name, e)
    # the control: finite, rounding noise and not another function
    c = R.swin_forward(sd, px, cfg, bf16_storage=True)
    for i, t in enumerate(c["outs"]):
        e = rel_l2(t, T(o[f"out.{i}"]))
        assert torch.isfinite(t).all() and 1e-4 < e < 5e-2, (geom, size, i, e)


def test_fixtures_exercise_what_they_claim():
    """50x38: patch pad on both axes, 13x10 padded to 14x14, odd grids into the merging, one stage equal to a window... : the geometry facts the
    issue lists, so a changed fixture cannot silently stop covering them."""
    assert 50 % 4 and 38 % 4
    assert stage_maps("a", (50, 38)) == [(13, 10), (7, 5), (4, 3)]          # 13x10 -> 14x14: 2x2 windows; 7x5: one (padded) window; 4x3: smaller than the window
    assert stage_maps("b", (90, 106)) == [(23, 27), (12, 14)]               # 23x27 -> 24x36: 2x3 windows
    assert stage_maps("b", (40, 40)) == [(10, 10), (5, 5)]                  # both smaller than the 12-window
    for g in TINY:
        sd = weights(g)
        tab = [v for k, v in sd.items() if k.endswith("relative_position_bias_table")]
        assert tab and all(0.3 < float(t.std()) < 0.7 for t in tab)        # re-drawn: the default 0.02 would hide a missing bias
        qb = [v for k, v in sd.items() if k.endswith("attn.qkv.bias")]
        assert qb and all(0.15 < float(t.std()) < 0.45 for t in qb)        # what pad tokens attend with


@pytest.mark.parametrize("geom", list(TINY))
def test_relative_position_index_equals_the_stored_buffer(geom):
    from anyedit_amd.groundingdino.swin_transformer import relative_position_index
    sd, ws = weights(geom), TINY[geom]["window_size"]
    keys = [k for k in sd if k.endswith("relative_position_index")]
    assert len(keys) == sum(TINY[geom]["depths"])
    for k in keys:
        assert torch.equal(relative_position_index(ws), sd[k]) and torch.equal(R.relative_position_index(ws), sd[k]), k


def _frames():
    """(Hp, Wp, ws) of every stage of every fixture image, plus Hp == ws on one and on both axes."""
    out = set()
    for g, s in CASES:
        ws = TINY[g]["window_size"]
        for h, w in stage_maps(g, s):
            out.add((R.up(h, ws), R.up(w, ws), ws))
    out |= {(7, 7, 7), (7, 21, 7), (12, 12, 12), (36, 12, 12)}
    return sorted(out)


def test_mask_formula_equals_the_slice_construction():
    frames = _frames()
    assert any(hp == ws for hp, _, ws in frames) and any(hp > 2 * ws for hp, _, ws in frames)
    for hp, wp, ws in frames:
        for shift in sorted({ws // 2, 1, ws - 1}):
            a, b = R.regions_by_formula(hp, wp, ws, shift), R.regions_by_slices(hp, wp, ws, shift)
            assert torch.equal(a, b), (hp, wp, ws, shift)
        if hp == ws:                                   # the first slice is empty: regions 0..2 along that axis never appear
            assert float(R.regions_by_formula(hp, wp, ws, ws // 2).min()) >= 3


def test_row_addressing_equals_pad_roll_partition():
    seen_pad = False
    for g, s in CASES:
        ws = TINY[g]["window_size"]
        for h, w in stage_maps(g, s) + [(ws, ws), (ws + 1, 2 * ws - 1), (3, 5), (2 * ws + 3, 3 * ws)]:
            for shift in (0, ws // 2):
                a, b = R.rows_by_formula(h, w, ws, shift), R.rows_by_partition(h, w, ws, shift)
                assert torch.equal(a, b), (h, w, ws, shift)
                real = a[a >= 0]
                assert real.numel() == h * w and torch.equal(real.sort().values, torch.arange(h * w))     # every image row exactly once
                seen_pad |= bool((a < 0).any())
    assert seen_pad


@pytest.mark.parametrize("geom", list(TINY))
def test_state_dict_keys_equal_the_fixtures(geom):
    sd = weights(geom)
    m = tower(geom)
    assert sorted(m.state_dict().keys()) == sorted(sd.keys())
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd, strict=True)
    assert m.eval() is m and m.train(False) is m


def test_a_wrong_index_buffer_is_refused():
    sd = weights("a")
    k = next(k for k in sd if k.endswith("relative_position_index"))
    sd[k] = sd[k].t().contiguous() + 1
    with pytest.raises(RuntimeError, match="relative position index"):
        tower("a").load_state_dict(sd, strict=True)


def test_load_groundingdino_backbone_takes_three_forms(tmp_path):
    from anyedit_amd.checkpoints import load_groundingdino_backbone
    sd = weights("a")
    other = {"transformer.level_embed": torch.zeros(4, 8), "bert.embeddings.word_embeddings.weight": torch.zeros(3, 8)}
    forms = {
        "swin": dict(sd),
        "groundingdino": {"model": dict({"backbone.0." + k: v for k, v in sd.items()}, **other)},
        "groundingdino-module": {"model": dict({"module.backbone.0." + k: v for k, v in sd.items()}, **{"module." + k: v for k, v in other.items()})},
    }
    for want, ck in forms.items():
        m = tower("a")
        assert load_groundingdino_backbone(m, ck) == want
        for k, v in m.state_dict().items():
            assert torch.equal(v.float(), sd[k].float()), (want, k)
    path = tmp_path / "gdino.pth"
    torch.save(forms["groundingdino"], path)
    m = tower("a")
    assert load_groundingdino_backbone(m, str(path)) == "groundingdino"
    assert torch.equal(m.layers[1].blocks[1].attn.qkv.bias, sd["layers.1.blocks.1.attn.qkv.bias"])
    broken = dict(sd)
    del broken["layers.0.downsample.reduction.weight"]
    with pytest.raises(RuntimeError, match="downsample.reduction.weight"):
        load_groundingdino_backbone(tower("a"), broken)


def test_constructor_refusals_and_geometries():
    from anyedit_amd.groundingdino.swin_transformer import SwinTransformer, build_swin_transformer, SWIN_GEOMETRIES
    with pytest.raises(ValueError, match="ape=True.*no GroundingDINO config sets it"):
        tower("a", ape=True)
    with pytest.raises(ValueError, match="head_dim 48/1.*head_dim 32 only"):
        SwinTransformer(embed_dim=48, depths=[2], num_heads=[1], out_indices=(0,))
    with pytest.raises(ValueError, match="window_size 17"):
        SwinTransformer(embed_dim=32, depths=[2], num_heads=[1], window_size=17, out_indices=(0,))
    with pytest.raises(ValueError, match="unknown model"):
        build_swin_transformer("swin_S_224_1k", 224)
    assert SWIN_GEOMETRIES == R.GEOMETRIES and len(SWIN_GEOMETRIES) == 5
    for name, g in SWIN_GEOMETRIES.items():          # head dim 32 at every stage of every geometry
        assert all(g["embed_dim"] * 2 ** i // h == 32 for i, h in enumerate(g["num_heads"])), name
    m = build_swin_transformer("swin_T_224_1k", 224, use_checkpoint=True, drop_path_rate=0.3, frozen_stages=2)
    assert m.num_features == [96, 192, 384, 768] and [len(l.blocks) for l in m.layers] == [2, 2, 6, 2]
    assert [l.downsample is not None for l in m.layers] == [True, True, True, False]
    assert not m.patch_embed.proj.weight.requires_grad and not m.layers[0].blocks[0].attn.qkv.weight.requires_grad and m.layers[1].blocks[0].attn.qkv.weight.requires_grad
    assert [b.shift_size for b in m.layers[2].blocks] == [0, 3, 0, 3, 0, 3]
    with pytest.raises(ValueError, match="stage 3 has head_dim 384/24"):      # dilation halves the last width, the table's head count then gives head_dim 16
        build_swin_transformer("swin_T_224_1k", 224, dilation=True)
    d = build_swin_transformer("swin_T_224_1k", 224, dilation=True, num_heads=[3, 6, 12, 12])
    assert d.num_features == [96, 192, 384, 384] and [l.downsample is not None for l in d.layers] == [True, True, False, False]
    assert d.stage_sizes(800, 800) == [(200, 200), (100, 100), (50, 50), (50, 50)] and m.stage_sizes(50, 38) == [(13, 10), (7, 5), (4, 3), (2, 2)]
    assert SWIN_GEOMETRIES["swin_T_224_1k"]["depths"] == [2, 2, 6, 2]     # the table is not mutated by a build
    with pytest.raises(ValueError, match="GPU only"):
        tower("a").forward_raw(torch.zeros(1, 3, 32, 32))


def test_the_library_exports_the_swin_symbols_and_refuses_bad_arguments():
    from anyedit_amd import _lib
    L = _lib.lib
    assert "ae_swin_window_attn_bf16" in _lib.SIGNATURES and "ae_swin_merge_ln_bf16" in _lib.SIGNATURES
    a, m = L.ae_swin_window_attn_bf16, L.ae_swin_merge_ln_bf16
    buf = (ctypes.c_uint16 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15                    # host memory: every call below must be refused before it is touched
    err = lambda: L.ae_last_error()
    # (qkv, ldq, qkv_bias, bias, out, ldo, B, H, W, C, nH, ws, shift, scale, stream)
    assert a(None, 96, p, p, p, 32, 1, 7, 7, 32, 1, 7, 0, 0.17, None) == -1 and b"null pointer" in err()
    assert a(p, 96, p, p, p, 32, 0, 7, 7, 32, 1, 7, 0, 0.17, None) == -1 and b"bad sizes" in err()
    assert a(p, 192, p, p, p, 64, 1, 7, 7, 64, 1, 7, 0, 0.17, None) == -1 and b"head_dim 64/1 must be 32" in err()
    assert a(p, 120, p, p, p, 40, 1, 7, 7, 40, 1, 7, 0, 0.17, None) == -1 and b"must be 32" in err()
    assert a(p, 96, p, p, p, 32, 1, 7, 7, 32, 1, 17, 0, 0.17, None) == -1 and b"window size 17" in err()
    assert a(p, 96, p, p, p, 32, 1, 7, 7, 32, 1, 0, 0, 0.17, None) == -1 and b"window size 0" in err()
    assert a(p, 96, p, p, p, 32, 1, 7, 7, 32, 1, 7, 7, 0.17, None) == -1 and b"shift 7" in err()
    assert a(p, 96, p, p, p, 32, 1, 7, 7, 32, 1, 7, -1, 0.17, None) == -1 and b"shift -1" in err()
    assert a(p, 88, p, p, p, 32, 1, 7, 7, 32, 1, 7, 0, 0.17, None) == -1 and b"qkv row stride" in err()
    assert a(p, 100, p, p, p, 32, 1, 7, 7, 32, 1, 7, 0, 0.17, None) == -1 and b"qkv row stride" in err()
    assert a(p, 96, p, p, p, 24, 1, 7, 7, 32, 1, 7, 0, 0.17, None) == -1 and b"out row stride" in err()
    assert a(p, 96, p, p + 8, p, 32, 1, 7, 7, 32, 1, 7, 0, 0.17, None) == -1 and b"aligned" in err()
    assert a(p, 96, p, p, p, 32, 4, 30000, 30000, 32, 1, 7, 0, 0.17, None) == -1 and b"2^31" in err()
    # (x, gamma, beta, y, B, H, W, C, eps, stream)
    assert m(p, p, None, p, 1, 4, 4, 32, 1e-5, None) == -1 and b"null pointer" in err()
    assert m(p, p, p, p, 1, 0, 4, 32, 1e-5, None) == -1 and b"bad sizes" in err()
    assert m(p, p, p, p, 1, 4, 4, 36, 1e-5, None) == -1 and b"multiple of 8" in err()
    assert m(p, p, p, p, 1, 4, 4, 1032, 1e-5, None) == -1 and b"is past 4096" in err()
    assert m(p, p + 4, p, p, 1, 4, 4, 32, 1e-5, None) == -1 and b"aligned" in err()


def _expected_shapes(cfg, out_indices=(0, 1, 2, 3)):
    """Key -> shape of the reference's state dict for a geometry of build_swin_transformer's table, from the class definitions (:108-131, :217-233,
    :311-312, :476-478, :629-632)."""
    ws, L = cfg["window_size"], len(cfg["depths"])
    want = {"patch_embed.proj.weight": (cfg["embed_dim"], 3, 4, 4), "patch_embed.proj.bias": (cfg["embed_dim"],),
            "patch_embed.norm.weight": (cfg["embed_dim"],), "patch_embed.norm.bias": (cfg["embed_dim"],)}
    for i in range(L):
        C, nH = cfg["embed_dim"] * 2 ** i, cfg["num_heads"][i]
        for j in range(cfg["depths"][i]):
            q = f"layers.{i}.blocks.{j}."
            for name, shape in (("norm1.weight", (C,)), ("norm1.bias", (C,)), ("attn.relative_position_bias_table", ((2 * ws - 1) ** 2, nH)),
                                ("attn.relative_position_index", (ws * ws, ws * ws)), ("attn.qkv.weight", (3 * C, C)), ("attn.qkv.bias", (3 * C,)),
                                ("attn.proj.weight", (C, C)), ("attn.proj.bias", (C,)), ("norm2.weight", (C,)), ("norm2.bias", (C,)),
                                ("mlp.fc1.weight", (4 * C, C)), ("mlp.fc1.bias", (4 * C,)), ("mlp.fc2.weight", (C, 4 * C)), ("mlp.fc2.bias", (C,))):
                want[q + name] = shape
        if i < L - 1:
            want[f"layers.{i}.downsample.reduction.weight"] = (2 * C, 4 * C)
            want[f"layers.{i}.downsample.norm.weight"], want[f"layers.{i}.downsample.norm.bias"] = (4 * C,), (4 * C,)
        if i in out_indices:
            want[f"norm{i}.weight"], want[f"norm{i}.bias"] = (C,), (C,)
    return want


@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_every_geometry_builds_with_the_reference_state_dict(name):
    """All five geometries of build_swin_transformer construct (on the meta device: Swin-L is 195 M parameters) with the reference's keys and
    shapes; GroundingDINO's out_indices = (1, 2, 3) drops norm0 only."""
    from anyedit_amd.groundingdino.swin_transformer import build_swin_transformer
    cfg = R.GEOMETRIES[name]
    with torch.device("meta"):
        m = build_swin_transformer(name, int(name.split("_")[-2]))
        m123 = build_swin_transformer(name, int(name.split("_")[-2]), out_indices=(1, 2, 3), dilation=False, use_checkpoint=True)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == _expected_shapes(cfg)
    assert {k: tuple(v.shape) for k, v in m123.state_dict().items()} == _expected_shapes(cfg, (1, 2, 3))
    assert m.num_features == [cfg["embed_dim"] * 2 ** i for i in range(4)] and m123.num_features == m.num_features
    assert [b.attn.num_heads for l in m.layers for b in l.blocks[:1]] == cfg["num_heads"]
