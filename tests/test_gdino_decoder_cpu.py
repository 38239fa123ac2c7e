"""CPU tests for the device code of GroundingDINO's query selection, decoder and heads: the restatements of tests/gdino_dec_ref.py against the
fixture the reference's own functions wrote (tests/golden/gdino_dec_geom.npz), the state-dict keys of the new module classes, the C-ABI symbols and
every refusal that is decided on the host before a launch.  No GPU is needed: a refused call returns before it touches a device."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, rel_l2, T  # noqa: E402
import gdino_dec_ref as R  # noqa: E402

NEW = ("ae_contrastive_bf16", "ae_topk_rows_max_n", "ae_topk_rows_f32", "ae_gdino_proposals_f32", "ae_gdino_query_sine", "ae_gdino_box_refine_f32")
P = 4096        # a non-null, 16-byte aligned address no refused call reads


def _refused(rc, needle):
    from anyedit_amd import _lib
    assert rc != 0, "the call was not refused"
    msg = _lib.lib.ae_last_error().decode()
    assert needle in msg, msg


def test_restatements_reproduce_the_reference_fixture():
    z = load_golden("gdino_dec_geom")
    levels = [tuple(int(v) for v in hw) for hw in z["spatial_shapes"]]
    assert (1, 1) in levels and any(h != w for h, w in levels)
    mask, ref = T(z["padding_mask"]), T(z["proposals"])
    mine, keep = R.encoder_output_proposals(mask, levels)
    assert torch.equal(torch.isposinf(mine), torch.isposinf(ref)), "the proposals' inf pattern"
    assert torch.equal(keep, T(z["memory_kept"])) and 0 < int(keep.sum()) < keep.numel()
    fin = torch.isfinite(ref)
    assert rel_l2(mine[fin], ref[fin]) <= 1e-5
    boxes = T(z["boxes"])
    assert bool((boxes == 0).any()) and bool((boxes == 1).any()) and bool((boxes == 0.5).any())
    assert rel_l2(R.query_sine_embed(boxes), T(z["sineembed"])) <= 1e-5
    x, y, m = T(z["ce_x"]), T(z["ce_y"]), T(z["ce_mask"])
    ce, want = R.contrastive(x, y, m, 16), T(z["ce_out"])
    assert torch.equal(torch.isneginf(ce), torch.isneginf(want)) and rel_l2(ce[torch.isfinite(want)], want[torch.isfinite(want)]) <= 1e-5
    assert bool(torch.isneginf(want[..., 12:]).all()) and bool(torch.isneginf(want[1, :, 7:]).all())


def test_restatement_details():
    # bf16 control of the one stored activation
    b = torch.rand(3, 4)
    e, eb = R.query_sine_embed(b), R.query_sine_embed(b, store=R.round_bf16)
    assert torch.equal(eb, e.to(torch.bfloat16).float()) and not torch.equal(eb, e)
    # inverse sigmoid: both clamps, and arguments outside [0, 1]
    x = torch.tensor([0.0, 1.0, 0.5, 5e-4, -0.2, 1.3])
    want = torch.log(torch.tensor([1e-3 / 1.0, 1.0 / 1e-3, 1.0, 1e-3 / (1 - 5e-4), 1e-3 / 1.0, 1.0 / 1e-3]))
    assert torch.allclose(R.inverse_sigmoid(x), want, rtol=1e-6, atol=1e-6)
    # the stable order torch.topk does not promise: ties by ascending index, NaN of either sign first, the two zeros equal
    v = torch.tensor([[1.0, float("nan"), 1.0, float("inf"), -0.0, 0.0, -float("nan"), float("-inf"), 1.0]])
    assert R.stable_topk(v, 9).tolist() == [[1, 6, 3, 0, 2, 8, 4, 5, 7]]
    # a fully padded sample: valid extents of 0, every proposal +inf
    p, keep = R.encoder_output_proposals(torch.ones(1, 6, dtype=torch.bool), [(2, 3)])
    assert bool(torch.isposinf(p).all()) and not keep.any()
    # reference_points_input and the +inf logit of a masked proposal
    rpi = R.reference_points_input(torch.ones(1, 2, 4), torch.tensor([[[0.5, 0.25], [1.0, 1.0]]]))
    assert rpi.shape == (1, 2, 2, 4) and rpi[0, 0, 0].tolist() == [0.5, 0.25, 0.5, 0.25]
    s, u = R.box_refine(torch.zeros(1, 256), torch.zeros(4, 256), torch.zeros(4), torch.full((1, 4), float("inf")), ref_is_logit=True)
    assert bool((s == 1).all()) and bool(torch.isposinf(u).all())


def test_module_classes_keep_the_references_state_dict_keys():
    from anyedit_amd.groundingdino import utils as U
    assert sorted(U.MLP(256, 256, 4, 3).state_dict()) == sorted(f"layers.{i}.{n}" for i in range(3) for n in ("weight", "bias"))
    m = U.MLP(512, 256, 256, 2)
    assert [tuple(l.weight.shape) for l in m.layers] == [(256, 512), (256, 256)] and m.num_layers == 2
    ce = U.ContrastiveEmbed(max_text_len=195)
    assert list(ce.state_dict()) == [] and ce.max_text_len == 195 and U.ContrastiveEmbed().max_text_len == 256
    x = torch.tensor([0.0, 1.0, 0.5, 5e-4, -0.2, 1.3, 0.3])
    assert torch.equal(U.inverse_sigmoid(x), R.inverse_sigmoid(x))


def test_module_refusals_before_any_launch():
    from anyedit_amd.groundingdino import utils as U
    with pytest.raises(NotImplementedError, match="learnedwh"):
        U.gen_encoder_output_proposals(torch.zeros(1, 4, 8), torch.zeros(1, 4, dtype=torch.bool), [(2, 2)], learnedwh=torch.zeros(2))
    with pytest.raises(NotImplementedError, match="2-d points"):
        U.gen_sineembed_for_position(torch.zeros(3, 1, 2))
    with pytest.raises(ValueError, match="Unknown pos_tensor"):
        U.gen_sineembed_for_position(torch.zeros(3, 1, 3))
    with pytest.raises(ValueError, match="GPU tensor"):                     # no CPU path, no eager fall-back
        U.ContrastiveEmbed()(torch.zeros(1, 2, 32), {"encoded_text": torch.zeros(1, 3, 32), "text_token_mask": torch.ones(1, 3, dtype=torch.bool)})
    with pytest.raises(ValueError, match="GPU tensor"):
        U.MLP(256, 256, 4, 3)(torch.zeros(2, 256))


def test_prediction_heads_checks_its_sequences_before_any_launch():
    from anyedit_amd.groundingdino import utils as U
    from anyedit_amd.groundingdino.transformer import prediction_heads
    hs, ref = [torch.zeros(1, 2, 256)] * 2, [torch.zeros(1, 2, 4)] * 3
    heads, cls, td = [U.MLP(256, 256, 4, 3)] * 2, [U.ContrastiveEmbed()] * 2, {}
    with pytest.raises(ValueError, match="need 3 references"):
        prediction_heads(hs, ref[:2], heads, cls, td)
    with pytest.raises(ValueError, match="box / class heads"):
        prediction_heads(hs, ref, heads[:1], cls, td)
    with pytest.raises(ValueError, match="0 decoder outputs"):
        prediction_heads([], ref[:1], heads, cls, td)


def test_c_abi_exports_the_new_entries():
    from anyedit_amd import _lib
    L = _lib.lib
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "anyedit_hip.h")).read()
    for name in NEW:
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"
    assert L.ae_topk_rows_max_n() >= 1 << 20


def test_contrastive_refuses_unsupported_sizes():
    from anyedit_amd import _lib
    f = _lib.lib.ae_contrastive_bf16
    ok = dict(x=P, ldx=256, y=P, m=None, lg=P, ldl=256, rm=P, B=1, N=5, Tn=12, C=256, L=256)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["ldx"], a["y"], a["m"], a["lg"], a["ldl"], a["rm"], a["B"], a["N"], a["Tn"], a["C"], a["L"], None)

    _refused(call(x=None), "null pointer")
    _refused(call(lg=None, rm=None), "neither logits nor rowmax")
    _refused(call(C=48, ldx=48), "multiple of 32")
    _refused(call(C=288, ldx=288), "at most 256")
    _refused(call(C=0), "multiple of 32")
    _refused(call(Tn=0), "1 <= T=0")
    _refused(call(Tn=13, L=12), "<= max_text_len=12")
    _refused(call(Tn=257, L=257), "<= 256")
    _refused(call(N=0), "bad sizes")
    _refused(call(ldx=128), "row stride of x")
    _refused(call(ldx=260), "multiple of 8")
    _refused(call(ldl=255), "row stride of logits")
    _refused(call(x=P + 2), "16-byte aligned")


def test_topk_refuses_unsupported_sizes():
    from anyedit_amd import _lib
    f = _lib.lib.ae_topk_rows_f32
    _refused(f(P, 2000, P, 1, 2000, 1025, None), "k=1025")
    _refused(f(P, 7, P, 1, 7, 8, None), "k=8")
    _refused(f(P, 7, P, 1, 7, 0, None), "k=0")
    _refused(f(P, 7, P, 1, 0, 1, None), "bad sizes")
    _refused(f(P, 6, P, 2, 7, 1, None), "row stride")
    _refused(f(P, 1 << 30, P, 1, _lib.lib.ae_topk_rows_max_n() + 1, 1, None), "largest supported row length")
    _refused(f(None, 7, P, 1, 7, 1, None), "null pointer")


def test_proposals_refuse_levels_that_do_not_tile_the_tokens():
    from anyedit_amd import _lib
    f = _lib.lib.ae_gdino_proposals_f32
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    _refused(f(P, ints(3, 3), ints(0), 1, P, P, 1, 12, None), "the levels hold 9 tokens")
    _refused(f(P, ints(3, 3, 2, 2), ints(0, 9), 2, P, P, 1, 12, None), "more than N=12")
    _refused(f(P, ints(3, 3, 1, 3), ints(0, 8), 2, P, P, 1, 12, None), "level 1 starts at 8")
    _refused(f(P, ints(0, 3), ints(0), 1, P, P, 1, 12, None), "shape (0, 3)")
    _refused(f(P, ints(*([1, 1] * 9)), ints(*range(9)), 9, P, P, 1, 9, None), "9 levels")
    _refused(f(None, ints(3, 4), ints(0), 1, P, P, 1, 12, None), "null pointer")
    _refused(f(P, ints(3, 4), ints(0), 1, P, P, 0, 12, None), "bad sizes")


def test_query_sine_and_box_refine_refuse_bad_arguments():
    from anyedit_amd import _lib
    q, r = _lib.lib.ae_gdino_query_sine, _lib.lib.ae_gdino_box_refine_f32
    _refused(q(P, P, P, P, 511, 1, 4, 1, None), "512 wide")
    _refused(q(P, P, P, P, 513, 1, 4, 1, None), "even")
    _refused(q(P, P, P, P, 512, 1, 0, 1, None), "bad sizes")
    _refused(q(P, P, P, P, 512, 1, 4, 65, None), "L at most 64")
    _refused(q(P, None, P, P, 512, 1, 4, 1, None), "null pointer")
    _refused(r(P, 255, P, P, P, P, None, 4, 0, None), "256 wide")
    _refused(r(P, 258, P, P, P, P, None, 4, 0, None), "multiple of 4")
    _refused(r(P, 256, P, P, P, P, None, 0, 0, None), "bad row count")
    _refused(r(P + 4, 256, P, P, P, P, None, 4, 0, None), "16-byte aligned")
    _refused(r(P, 256, P, None, P, P, None, 4, 0, None), "null pointer")


# ------------------------------------------------------------------------------------------------------------------ the tower
def _cmp_all(mine, io, prefix=""):
    n = 0
    for k, want in io.items():
        if not torch.is_tensor(want) or not k.startswith(prefix) or k[len(prefix):] not in mine or (not prefix and k.startswith("no.")):
            continue
        got = mine[k[len(prefix):]]
        if not want.dtype.is_floating_point:
            assert torch.equal(got.to(want.dtype), want), k
        else:
            fin = torch.isfinite(want)
            assert torch.equal(torch.isfinite(got), fin), k
            assert rel_l2(got[fin], want[fin]) <= 1e-5, (k, rel_l2(got[fin], want[fin]))
        n += 1
    return n


def test_tower_restatement_reproduces_every_stored_tensor():
    io, sd = R.tower_io(), R.tower_weights()
    srcs, masks, _, text, tm = R.tower_inputs(io)
    free = R.transformer_forward(sd, R.GEOM, srcs, masks, text, tm)["topk_proposals"]
    stored_idx = io["topk_proposals"]
    for b in range(stored_idx.shape[0]):                            # the stored indices, exactly — but torch.topk promises no order among the exactly
        sc = io["topk_logits"][b][stored_idx[b]]                    # tied masked rows, so slots that share a score are compared as a set
        tied = (sc[:, None] == sc[None, :]).sum(1) > 1
        assert torch.equal(free[b][~tied], stored_idx[b][~tied]), "the stored indices"
        assert sorted(free[b][tied].tolist()) == sorted(stored_idx[b][tied].tolist()), "the tied slots hold the same rows"
    mine = R.transformer_forward(sd, R.GEOM, srcs, masks, text, tm, topk_proposals=stored_idx)
    assert _cmp_all(mine, io) == 7 + 3 * 2 + 2 * 2               # scores, indices, the five outputs; three taps and two head outputs per layer
    mine_no = R.transformer_forward(sd, R.GEOM, srcs, masks, text, tm, two_stage="no")
    assert _cmp_all(mine_no, io, "no.") == 3 + 3 * 2 + 2 * 2
    # what the generator asserted: a gap behind the last slot, and masked rows among the selected of sample 1
    nq = R.GEOM["num_queries"]
    srt = torch.sort(io["topk_logits"], 1, descending=True)[0]
    assert float((srt[:, nq - 1] - srt[:, nq]).min()) > 1e-3
    _, keep = R.encoder_output_proposals(torch.cat([m.flatten(1) for m in masks], 1), R.GEOM["levels"])
    assert int((~keep[1][io["topk_proposals"][1]]).sum()) >= 1
    # the bf16 control differs from the fp32 run and stays close to it
    ctl = R.transformer_forward(sd, R.GEOM, srcs, masks, text, tm, store=R.round_bf16, topk_proposals=io["topk_proposals"])
    assert 0 < rel_l2(ctl["hs"], io["hs"]) < 5e-2


def test_tower_modules_keep_the_goldens_state_dict_keys():
    io = R.tower_io()
    for two_stage, keys in (("standard", io["keys"]), ("no", io["no.keys"])):
        m = R.tower_module(two_stage)
        assert sorted(m.state_dict()) == sorted(str(k) for k in keys), two_stage
    assert m.decoder.bbox_embed[0] is m.decoder.bbox_embed[1]


def test_loader_takes_three_forms_and_is_strict():
    from anyedit_amd.checkpoints import load_groundingdino_transformer
    m = R.tower_module()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    other = {"bbox_embed.0.layers.0.weight": torch.zeros(256, 256), "backbone.0.norm1.weight": torch.zeros(3), "transformer_not.x": torch.zeros(1)}
    forms = {"transformer": sd, "groundingdino": {"model": dict({"transformer." + k: v for k, v in sd.items()}, **other)},
             "groundingdino-module": dict({"module.transformer." + k: v for k, v in sd.items()}, **{"module." + k: v for k, v in other.items()})}
    for want, ck in forms.items():
        fresh = R.tower_module()
        with torch.no_grad():
            for p in fresh.parameters():
                p.zero_()
        assert load_groundingdino_transformer(fresh, ck) == want
        for k, v in fresh.state_dict().items():
            assert torch.equal(v, sd[k]), (want, k)
    short = dict(sd)
    del short["decoder.layers.1.ca_text.in_proj_bias"]
    with pytest.raises(KeyError, match=r"decoder\.layers\.1\.ca_text\.in_proj_bias"):
        load_groundingdino_transformer(m, short)
    extra = dict({"transformer." + k: v for k, v in sd.items()}, **{"transformer.decoder.layers.0.norm4.weight": torch.zeros(256)})
    with pytest.raises(KeyError, match=r"decoder\.layers\.0\.norm4\.weight"):
        load_groundingdino_transformer(m, extra)


def test_transformer_refuses_what_is_not_built():
    from anyedit_amd.groundingdino.transformer import Transformer, TransformerDecoder, DeformableTransformerDecoderLayer, build_transformer
    base = dict(num_encoder_layers=0, num_decoder_layers=1, dim_feedforward=64, return_intermediate_dec=True, learnable_tgt_init=True, num_queries=4)
    with pytest.raises(ValueError, match="must be 256"):
        Transformer(d_model=128, nhead=4, **base)
    with pytest.raises(NotImplementedError, match="num_patterns"):
        Transformer(num_patterns=2, **base)
    with pytest.raises(NotImplementedError, match="two_stage_type"):
        Transformer(two_stage_type="early", **base)
    with pytest.raises(ValueError, match="head_dim"):
        DeformableTransformerDecoderLayer(256, 64, n_heads=4)
    with pytest.raises(NotImplementedError, match="query_dim 2"):
        TransformerDecoder(DeformableTransformerDecoderLayer(256, 64), 1, torch.nn.LayerNorm(256), return_intermediate=True, query_dim=2)
    m = R.tower_module()
    io = R.tower_io()
    srcs, masks, poss, text, tm = R.tower_inputs(io)
    td = {"encoded_text": text, "text_token_mask": tm}
    for kw in (dict(refpoint_embed=torch.zeros(2, 3, 4)), dict(tgt=torch.zeros(2, 3, 256)), dict(attn_mask=torch.zeros(23, 23, dtype=torch.bool))):
        a = dict(dict(refpoint_embed=None, tgt=None, attn_mask=None), **kw)
        with pytest.raises(NotImplementedError, match="denoising"):
            m(srcs, masks, a["refpoint_embed"], poss, a["tgt"], a["attn_mask"], td)
    drop = Transformer(dropout=0.1, **base).requires_grad_(False).train()
    with pytest.raises(RuntimeError, match="non-zero dropout"):
        drop(srcs, masks, None, poss, None, None, td)
    grad = Transformer(**base)
    with pytest.raises(RuntimeError, match="inference only"):
        grad(srcs, masks, None, poss, None, None, td)
    nohead = Transformer(two_stage_type="standard", num_feature_levels=3, **base).requires_grad_(False).eval()
    import types
    args = types.SimpleNamespace(hidden_dim=256, dropout=0.0, nheads=8, num_queries=900, dim_feedforward=2048, enc_layers=6, dec_layers=6, pre_norm=False,
                                 query_dim=4, transformer_activation="relu", num_patterns=0, num_feature_levels=4, enc_n_points=4, dec_n_points=4,
                                 two_stage_type="standard", embed_init_tgt=True, use_text_enhancer=True, use_fusion_layer=True, use_checkpoint=True,
                                 use_transformer_ckpt=True, use_text_cross_attention=True, text_dropout=0.0, fusion_dropout=0.0, fusion_droppath=0.1)
    full = build_transformer(args)
    assert len(full.decoder.layers) == 6 and len(full.encoder.fusion_layers) == 6 and full.tgt_embed.weight.shape == (900, 256) and full.level_embed.shape == (4, 256)
    assert nohead.enc_out_bbox_embed is None
