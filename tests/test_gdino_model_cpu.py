"""CPU tests of the GroundingDINO detector's host side: the neck restatement against the reference's own outputs (tests/golden/gdino_neck.npz),
the model's state-dict names, the strict loader, the phrase helpers and the header declarations."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, rel_l2, T  # noqa: E402
import gdino_model_ref as MR  # noqa: E402
import gdino_neck_ref as NR  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_neck_restatement_reproduces_the_reference_fixture():
    g = {k: T(v) for k, v in load_golden("gdino_neck").items()}
    mask = g["mask"]
    for l, (h, w) in enumerate(g["shapes"].tolist()):
        lm = NR.level_mask(mask, h, w)
        assert torch.equal(lm, g[f"lmask.{l}"]), f"level {l}: the integer resize differs from F.interpolate"
        vw, vh = NR.valid_counts(lm)
        assert torch.equal(vw, (~g[f"lmask.{l}"][:, 0, :]).sum(1)) and torch.equal(vh, (~g[f"lmask.{l}"][:, :, 0]).sum(1))
        assert torch.equal(NR.valid_ratio(lm), g[f"vr.{l}"]), f"level {l}: valid ratios"
        pos = NR.position_sine(lm, 128, 20, 20, torch.float32).permute(0, 3, 1, 2)
        assert rel_l2(pos, g[f"pos.{l}"]) <= 1e-6, f"level {l}: sine embedding"
        assert rel_l2(NR.position_sine(lm, 128, 20, 20, torch.float64).permute(0, 3, 1, 2), g[f"pos.{l}"]) <= 1e-6
    assert bool(g["lmask.0"][2].all(0).any()) and bool(g["lmask.0"][2].all(1).any()), "the fixture holds a fully padded column and row"
    for name, stride in (("proj1", 1), ("proj2", 2)):
        y = NR.input_proj(g[name + ".x"], g[name + ".w"], g[name + ".b"], g[name + ".g"], g[name + ".e"], stride)
        assert rel_l2(y, g[name + ".y"]) <= 1e-6, name


def test_level_geometry_restatement_concatenates_the_levels():
    g = {k: T(v) for k, v in load_golden("gdino_neck").items()}
    shapes = [tuple(s) for s in g["shapes"].tolist()]
    le = torch.randn(4, 256, generator=torch.Generator().manual_seed(0))
    mf, pf, vr, counts = NR.level_geometry(g["mask"], shapes, 20, 20, le, torch.float32)
    st = 0
    for l, (h, w) in enumerate(shapes):
        assert torch.equal(mf[:, st:st + h * w].view(3, h, w), g[f"lmask.{l}"])
        want = g[f"pos.{l}"].permute(0, 2, 3, 1).reshape(3, h * w, 256) + le[l]
        assert rel_l2(pf[:, st:st + h * w], want) <= 1e-6
        assert torch.equal(vr[:, l], g[f"vr.{l}"])
        assert torch.equal(counts[l][0][:, -1], (~g[f"lmask.{l}"]).sum(1)) and torch.equal(counts[l][1][:, :, -1], (~g[f"lmask.{l}"]).sum(2))
        st += h * w


def test_ground_restatement_keeps_query_order():
    lg = torch.tensor([[0.0, -9.0], [2.0, -float("inf")], [-9.0, -9.0], [-float("inf"), 1.0]])
    idx, score, boxes, pm = NR.ground(lg, torch.arange(16.0).view(4, 4), 0.3, 0.6)
    assert idx.tolist() == [0, 1, 3] and pm.tolist() == [[False, False], [True, False], [False, True]]
    assert torch.equal(boxes, torch.arange(16.0).view(4, 4)[[0, 1, 3]]) and torch.allclose(score, torch.tensor([0.5, 0.8808, 0.7311]), atol=1e-4)


# ------------------------------------------------------------------------------------------------------------------ names
def _swinb_args():
    return types.SimpleNamespace(
        backbone="swin_B_384_22k", position_embedding="sine", pe_temperatureH=20, pe_temperatureW=20, return_interm_indices=[1, 2, 3],
        backbone_freeze_keywords=None, hidden_dim=256, dropout=0.0, nheads=8, num_queries=900, dim_feedforward=2048, enc_layers=6, dec_layers=6,
        pre_norm=False, query_dim=4, transformer_activation="relu", num_patterns=0, num_feature_levels=4, enc_n_points=4, dec_n_points=4,
        two_stage_type="standard", embed_init_tgt=True, use_text_enhancer=True, use_fusion_layer=True, use_checkpoint=True, use_transformer_ckpt=True,
        use_text_cross_attention=True, text_dropout=0.0, fusion_dropout=0.0, fusion_droppath=0.1, dec_pred_bbox_embed_share=True,
        two_stage_bbox_embed_share=False, two_stage_class_embed_share=False, dn_box_noise_scale=1.0, dn_label_noise_ratio=0.5, dn_labelbook_size=2000,
        text_encoder_type="bert-base-uncased", sub_sentence_present=True, max_text_len=256)


def test_state_dict_names_of_the_swinb_config():
    """GroundingDINO_SwinB_cfg.py: exactly backbone.0.*, transformer.*, bert.*, feat_map.*, input_proj.<l>.{0,1}.{weight,bias} for four levels and
    bbox_embed.<i>.layers.<j>.* for six decoder layers; the shared box head under every alias."""
    from anyedit_amd.groundingdino.groundingdino import build_groundingdino
    with torch.device("meta"):
        m = build_groundingdino(_swinb_args(), tokenizer=MR.StandInTokenizer())
    keys = list(m.state_dict().keys())
    assert {k.split(".")[0] for k in keys} == {"backbone", "transformer", "bert", "feat_map", "input_proj", "bbox_embed"}
    assert all(k.startswith("backbone.0.") for k in keys if k.startswith("backbone."))
    assert sorted(k for k in keys if k.startswith("input_proj.")) == sorted(f"input_proj.{l}.{i}.{n}" for l in range(4) for i in (0, 1) for n in ("weight", "bias"))
    assert sorted(k for k in keys if k.startswith("bbox_embed.")) == sorted(f"bbox_embed.{i}.layers.{j}.{n}" for i in range(6) for j in range(3) for n in ("weight", "bias"))
    assert sorted(k for k in keys if k.startswith("feat_map.")) == ["feat_map.bias", "feat_map.weight"]
    assert tuple(m.input_proj[0][0].weight.shape) == (256, 256, 1, 1) and tuple(m.input_proj[2][0].weight.shape) == (256, 1024, 1, 1)
    assert tuple(m.input_proj[3][0].weight.shape) == (256, 1024, 3, 3) and m.input_proj[3][0].stride == (2, 2)
    for i in range(6):
        assert f"transformer.decoder.bbox_embed.{i}.layers.2.weight" in keys
        assert m.transformer.decoder.bbox_embed[i] is m.bbox_embed[0]
    assert "transformer.enc_out_bbox_embed.layers.0.weight" in keys and m.transformer.enc_out_bbox_embed is not m.bbox_embed[0]
    assert "transformer.level_embed" in keys and "bert.embeddings.word_embeddings.weight" in keys and "bert.pooler.dense.weight" in keys
    assert m.specical_tokens == [1, 2, 3, 4] and m.level_sizes(800, 1200) == [(100, 150), (50, 75), (25, 38), (13, 19)]


def test_head_sharing_follows_the_three_flags():
    m = MR.tiny_model()
    sd = m.state_dict()
    a, b = sd["bbox_embed.0.layers.0.weight"], sd["transformer.decoder.bbox_embed.1.layers.0.weight"]
    assert a.data_ptr() == b.data_ptr() == sd["bbox_embed.1.layers.0.weight"].data_ptr(), "the aliases of a shared head must share storage"
    assert sd["transformer.enc_out_bbox_embed.layers.0.weight"].data_ptr() != a.data_ptr(), "two_stage_bbox_embed_share=False is a copy"
    assert m.transformer.decoder.class_embed is m.class_embed and m.transformer.enc_out_class_embed is not m.class_embed[0]
    assert {k.split(".")[0] for k in sd} == {"backbone", "transformer", "bert", "feat_map", "input_proj", "bbox_embed"}


def test_refusals():
    from anyedit_amd.groundingdino.backbone import build_backbone
    from anyedit_amd.groundingdino.position_encoding import build_position_encoding
    args = _swinb_args()
    args.position_embedding = "learned"
    with pytest.raises(NotImplementedError, match="learned"):
        build_position_encoding(args)
    args = _swinb_args()
    args.backbone = "resnet50"
    with pytest.raises(NotImplementedError, match="resnet50"):
        build_backbone(args)
    m = MR.tiny_model()
    with pytest.raises(NotImplementedError, match="targets"):
        m(torch.zeros(1, 3, 8, 8), targets=[{"caption": "cat ."}])
    with pytest.raises(ValueError, match="captions"):
        m(torch.zeros(1, 3, 8, 8))


# ------------------------------------------------------------------------------------------------------------------ the loader
def test_load_groundingdino_round_trips_and_is_strict():
    from anyedit_amd.checkpoints import load_groundingdino
    sd = dict(MR.tiny_state_dict())
    m = MR.tiny_model()
    for k, v in m.state_dict().items():
        if k in sd:
            assert torch.equal(v.float(), sd[k].float()), k
    public = dict(sd)
    public["bert.embeddings.position_ids"] = torch.arange(64)[None]
    public["label_enc.weight"] = torch.zeros(3, 256)
    assert load_groundingdino(m, {"model": {"module." + k: v for k, v in public.items()}}) == "checkpoint-module"
    assert load_groundingdino(m, public) == "state_dict"
    with pytest.raises(KeyError, match="input_proj.2.0.weight"):
        load_groundingdino(m, {k: v for k, v in sd.items() if k != "input_proj.2.0.weight"})
    with pytest.raises(KeyError, match="no place"):
        load_groundingdino(m, dict(sd, **{"input_proj.9.0.weight": torch.zeros(1)}))


# ------------------------------------------------------------------------------------------------------------------ phrases
def test_caption_and_phrase_helpers():
    from anyedit_amd.groundingdino import inference as I
    assert I.preprocess_caption("  A Cat ") == "a cat." and I.preprocess_caption("dog .") == "dog ."
    tok = MR.StandInTokenizer()
    tokenized = tok("cat . red dog .")
    assert tokenized["input_ids"] == [1, 10, 3, 13, 11, 3, 2]
    pm = torch.zeros(256, dtype=torch.bool)
    pm[3], pm[4] = True, True
    assert I.get_phrases_from_posmap(pm, tokenized, tok) == "red dog"
    assert I.get_phrases_from_posmap(torch.zeros(256, dtype=torch.bool), tokenized, tok) == ""
    with pytest.raises(NotImplementedError):
        I.get_phrases_from_posmap(pm[None], tokenized, tok)
    assert I.format_phrase("red dog", 0.4567891) == "red dog(0.45)" and I.format_phrase("red dog", 0.4567891, with_logits=False) == "red dog"
    bits = torch.tensor([[5, 0], [-2 ** 31, 1]], dtype=torch.int32)
    p = I.posmaps_from_bits(bits, 64)
    assert p[0].nonzero().flatten().tolist() == [0, 2] and p[1].nonzero().flatten().tolist() == [31, 32]
    assert I.resized_size(640, 480) == (800, 1066) and I.resized_size(480, 640) == (1066, 800) and I.resized_size(2000, 500) == (333, 1332)


def test_load_image_tensor():
    from PIL import Image
    from anyedit_amd.groundingdino import inference as I
    x = I.load_image_tensor(Image.new("RGB", (64, 48), (255, 0, 128)))
    assert tuple(x.shape) == (3, 800, 1066) and x.dtype == torch.float32
    want = (torch.tensor([1.0, 0.0, 128 / 255]) - torch.tensor(I.IMAGENET_MEAN)) / torch.tensor(I.IMAGENET_STD)
    assert torch.allclose(x[:, 5, 7], want, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ the C interface
def test_every_neck_entry_is_declared_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "anyedit_hip.h")).read()
    lib_py = open(os.path.join(ROOT, "anyedit_amd", "_lib.py")).read()
    ops_py = open(os.path.join(ROOT, "anyedit_amd", "ops.py")).read()
    for name in ("ae_gdino_level_geometry", "ae_gdino_neck_groupnorm_workspace_floats", "ae_gdino_neck_groupnorm", "ae_gdino_ground"):
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"
        assert f'"{name}"' in lib_py, f"{name} is not bound in _lib.py"
        assert f"lib.{name}(" in ops_py, f"{name} is not called from ops.py"
    assert "gdino_neck.hip" in open(os.path.join(ROOT, "anyedit_amd", "build.py")).read()
    for ref in ("position_encoding.py:98-131", "backbone.py:113", "groundingdino.py:306", "groundingdino.py:127-138", "tool.py:125-133"):
        assert ref in header, f"the header does not name the reference lines {ref}"
