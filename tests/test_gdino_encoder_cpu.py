"""Host-side checks of GroundingDINO's feature enhancer (no GPU): the chain of trust of its fixtures (the restatement against every stored
output and every per-sub-block stream), the sine position embedding, the state-dict key schema against the reference's key list, the three
checkpoint forms with their strictness, the constructors' refusals and the C ABI's exports.  The modules are constructed on the CPU: nothing here
launches a kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, rel_l2, T  # noqa: E402
import gdino_enc_ref as R  # noqa: E402

GEOMS, weights, stored, module, run_restatement = R.GEOMS, R.weights, R.stored, R.module, R.run_restatement


@pytest.mark.parametrize("geom", list(GEOMS))
def test_fixture_inputs_are_what_the_issue_asks_for(geom):
    g, o = GEOMS[geom], stored(geom)
    n_img = sum(h * w for h, w in g["levels"])
    assert o["src"].shape == (2, n_img, g["d_model"]) and o["memory_text"].shape == (2, 12, g["d_model"])
    kpm, tm, ts = T(o["key_padding_mask"]), T(o["text_attention_mask"]), T(o["text_self_attention_masks"])
    assert not bool(kpm[0].any()) and bool(kpm[1].any()) and not bool(kpm[1].all())
    assert float(T(o["valid_ratios"])[1].max()) < 1.0
    assert int((~tm[1]).sum()) == 7 and not bool(tm[0].any())
    assert not torch.equal(ts[0], ts[1]) and bool(torch.diagonal(ts, dim1=1, dim2=2).all())
    assert T(o["spatial_shapes"]).tolist() == [list(s) for s in g["levels"]]


@pytest.mark.parametrize("geom", list(GEOMS))
def test_restatement_matches_the_reference_golden(geom):
    """tests/gdino_enc_ref.py (fp32) against what the reference's TransformerEncoder produced: rel-L2 <= 1e-5 (the Swin figure, fp32 against
    fp32) on both outputs and on the stream every sub-block of every layer leaves (measured at generation: 2e-7 .. 5e-7)."""
    o = stored(geom)
    taps = {}

    def tap(i, name, x, t):
        if name in ("fusion", "deform"):
            taps[f"tap.{i}.{name}.v"] = x
        if name in ("fusion", "text"):
            taps[f"tap.{i}.{name}.l"] = t

    out, out_text = run_restatement(geom, tap=tap)
    got = dict(taps, out=out, out_text=out_text)
    assert sorted(got) == sorted(k for k in o if k.startswith("tap.") or k in ("out", "out_text")), "every stored stream is checked"
    assert len(taps) == 4 * GEOMS[geom]["num_layers"]
    for name, v in got.items():
        e = rel_l2(v, T(o[name]))
        assert e <= 1e-5, (geom, name, e)
    # the control: finite, rounding noise and not another function
    c_out, c_text = run_restatement(geom, store=R.round_bf16)
    for name, c, r in (("out", c_out, out), ("out_text", c_text, out_text)):
        e = rel_l2(c, r)
        assert torch.isfinite(c).all() and 1e-4 < e < 5e-2, (geom, name, e)


def test_repeat_indexing_is_pinned_by_geometry_b():
    """With 2 text heads and different masks per sample, reading slice b * nhead + h as sample b's mask (what nn.MultiheadAttention's layout
    suggests) instead of sample (b * nhead + h) mod bs (what the reference's `repeat` gives) must miss the golden."""
    o = stored("b")
    real = R.expand_allowed
    try:
        R.expand_allowed = lambda allowed, nhead: allowed.repeat_interleave(nhead, 0)
        _, wrong = run_restatement("b")
    finally:
        R.expand_allowed = real
    assert rel_l2(wrong, T(o["out_text"])) > 1e-3


def test_sine_position_embedding_matches_its_golden():
    from anyedit_amd.groundingdino.utils import get_sine_pos_embed
    s = load_golden("gdino_enc_sine")
    ids, want = T(s["position_ids"]), T(s["embed"])
    assert ids.shape == (2, 12) and want.shape == (2, 12, 256)
    assert rel_l2(R.sine_pos_embed(ids[..., None], 256, exchange_xy=False), want) <= 1e-6
    assert rel_l2(get_sine_pos_embed(ids[..., None], num_pos_feats=256, exchange_xy=False), want) <= 1e-6
    xy = torch.rand(2, 5, 2)
    assert rel_l2(get_sine_pos_embed(xy, 64), R.sine_pos_embed(xy, 64)) <= 1e-6            # exchange_xy defaults to True in both
    assert torch.equal(get_sine_pos_embed(xy, 64)[..., :64], get_sine_pos_embed(xy, 64, exchange_xy=False)[..., 64:])


@pytest.mark.parametrize("geom", list(GEOMS))
def test_state_dict_keys_are_the_reference_s(geom):
    keys = [str(k) for k in stored(geom)["keys"]]
    m = module(geom)
    assert sorted(m.state_dict().keys()) == sorted(keys)
    assert "text_layers.0.self_attn.in_proj_weight" in keys and "fusion_layers.0.gamma_v" in keys
    sd = weights(geom)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_load_groundingdino_encoder_takes_three_forms_and_is_strict():
    from anyedit_amd.checkpoints import load_groundingdino_encoder
    sd = weights("a")
    other = {"backbone.0.patch_embed.proj.weight": torch.zeros(1), "bert.embeddings.word_embeddings.weight": torch.zeros(1),
             "transformer.decoder.norm.weight": torch.zeros(1), "transformer.level_embed": torch.zeros(1)}
    forms = {"encoder": dict(sd),
             "groundingdino": {"model": dict({"transformer.encoder." + k: v for k, v in sd.items()}, **other)},
             "groundingdino-module": dict({"module.transformer.encoder." + k: v for k, v in sd.items()}, **{"module." + k: v for k, v in other.items()})}
    for want, ck in forms.items():
        m = module("a")
        assert load_groundingdino_encoder(m, ck) == want
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), (want, k)
    m = module("a")
    short = dict(sd)
    del short["fusion_layers.1.gamma_l"]
    with pytest.raises(KeyError, match=r"fusion_layers\.1\.gamma_l"):
        load_groundingdino_encoder(m, short)
    extra = dict({"transformer.encoder." + k: v for k, v in sd.items()}, **{"transformer.encoder.layers.0.norm3.weight": torch.zeros(64)})
    with pytest.raises(KeyError, match=r"layers\.0\.norm3\.weight"):
        load_groundingdino_encoder(m, extra)


def test_constructors_refuse_what_is_not_built():
    from anyedit_amd.groundingdino.fuse_modules import BiAttentionBlock, BiMultiHeadAttention
    from anyedit_amd.groundingdino.transformer import DeformableTransformerEncoderLayer, build_feature_enhancer
    from anyedit_amd.groundingdino.transformer_vanilla import TransformerEncoderLayer
    from anyedit_amd.groundingdino.utils import _get_activation_fn, _get_clones
    with pytest.raises(ValueError, match="head_dim 256"):
        BiMultiHeadAttention(64, 64, 512, 4)                      # head_dim 128
    with pytest.raises(ValueError, match="head_dim 256"):
        BiAttentionBlock(256, 256, 2048, 4)                       # head_dim 512
    with pytest.raises(ValueError, match="32 or 64"):
        TransformerEncoderLayer(256, 2)                           # head_dim 128
    for act in ("gelu", "glu", "prelu", "selu"):
        with pytest.raises(NotImplementedError, match=act):
            _get_activation_fn(act)
        with pytest.raises(NotImplementedError, match=act):
            DeformableTransformerEncoderLayer(64, 128, activation=act, n_levels=1, n_heads=2)
    with pytest.raises(RuntimeError, match="relu/gelu"):
        _get_activation_fn("tanh")
    m = build_feature_enhancer()                                  # the production geometry
    assert len(m.layers) == len(m.text_layers) == len(m.fusion_layers) == 6
    assert m.text_layers[0].nhead == 4 and m.text_layers[0].linear1.out_features == 1024
    assert m.fusion_layers[0].attn.embed_dim == 1024 and m.fusion_layers[0].attn.num_heads == 4 and m.layers[0].self_attn.num_heads == 8
    clones = _get_clones(m.text_layers[0], 2)
    assert clones[0] is not clones[1] and clones[0].linear1.weight.data_ptr() != clones[1].linear1.weight.data_ptr()
    shared = _get_clones(m.text_layers[0], 2, layer_share=True)
    assert shared[0] is shared[1]


def test_forward_refuses_training_and_gradients_before_any_launch():
    m = module("a")
    x = torch.zeros(1, 4, 64)
    with pytest.raises(RuntimeError, match="inference only"):
        m.fusion_layers[0].eval()(x, x)                           # parameters require grad and grad mode is on
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="non-zero dropout"):
            m.fusion_layers[0].train()(x, x)                      # fusion dropout 0.1
        with pytest.raises(RuntimeError, match="non-zero dropout"):
            m.text_layers[0].train()(x.transpose(0, 1), torch.zeros(1, 4, 4, dtype=torch.bool))


def test_expand_text_mask_reproduces_repeat():
    from anyedit_amd.groundingdino.transformer_vanilla import expand_text_mask
    allowed = torch.rand(3, 5, 5) > 0.5
    for nhead in (1, 2, 4):
        got = expand_text_mask(allowed, nhead)
        assert got.dtype == torch.uint8 and torch.equal(got.bool(), allowed.repeat(nhead, 1, 1))     # the reference's own call
        assert torch.equal(got.bool(), R.expand_allowed(allowed, nhead))


def test_c_abi_exports_the_new_entries_and_plans_the_split():
    from anyedit_amd import _lib
    L = _lib.lib
    for name in ("ae_biattn_bf16", "ae_biattn_workspace_bytes", "ae_biattn_split_rows", "ae_attn_masked_short_bf16", "ae_scale_residual_f32_bf16"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.ae_biattn_workspace_bytes(1, 4, 13294, 256, 128) == 0 and L.ae_biattn_workspace_bytes(1, 4, 13294, 257, 256) == 0
    for nv in (1, 64, 65, 128, 129, 300, 13294, 1 << 20):
        rows = L.ae_biattn_split_rows(nv)
        nsplit = -(-nv // rows)
        assert rows % 64 == 0 and 1 <= nsplit <= 32, (nv, rows)
        assert L.ae_biattn_workspace_bytes(2, 4, nv, 200, 256) == 2 * 4 * nsplit * 200 * 258 * 4     # bounded by 32 partials: nothing grows with Nv * Nt
    assert L.ae_biattn_bf16(None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, 1, 1, 1, 1, 256, 1.0, None, 0, None) != 0
    assert b"null pointer" in L.ae_last_error()
