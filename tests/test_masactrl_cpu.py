"""MasaCtrl on the CPU: the float64 statements of tests/masactrl_ref.py and the editor classes of anyedit_amd.masactrl against the reference's
own outputs (tests/golden/masactrl.npz, written by tools/gen_golden_masactrl.py from the reference's editor classes in fp32).

Tolerance of the pin.  The golden is fp32: logits of up to ~20 (|q| |k| scale at the stored operands, queries scaled by up to 1.5) carry an
absolute error of ~8 products x 2^-24 x 20 = 1e-5, which is the relative error of a probability; an output is sum_j p_j v_j with sum p = 1 and
|v| <= ~4, so |golden - float64| stays below a few 1e-5.  5e-5 absolute is asserted; a wrong gate, source sample or class moves an output by
1e-1 and more."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import masactrl_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "masactrl.npz")
TOL = 5e-5


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


def _bhnd(t):
    """(b h) n d -> [B, H, n, D] float64"""
    return t.reshape(R.G_B, R.G_H, t.shape[1], t.shape[2]).to(R.F64)


def _rows_out(r):
    """[B, H, N, D] -> [B, rows, H D] at the golden's rows"""
    return r.permute(0, 2, 1, 3).reshape(R.G_B, r.shape[2], -1)[:, list(R.G_ROWS)]


def _mask_classes(name):
    ms, mt = R.golden_masks(name)
    ks = F.interpolate(ms[None, None], (16, 16)).flatten().to(torch.uint8)
    qt = F.interpolate(mt[None, None], (16, 16)).flatten().to(torch.uint8)
    qcls = torch.full((4, R.G_N), R.CLS_ANY, dtype=torch.uint8)
    qcls[1] = qt
    qcls[3] = qt
    return qcls, ks[None].repeat(4, 1)


def test_golden_masks_hold_the_edge_cases():
    _, k = _mask_classes("mask_empty")
    assert int(k[0].sum()) == 0                               # an empty foreground class ...
    q, _ = _mask_classes("mask_empty")
    assert int((q[1] == 1).sum()) > 0                         # ... that target queries do ask for
    _, k = _mask_classes("mask_one")
    assert int(k[0].sum()) == 1                               # a single foreground key
    q, k = _mask_classes("mask")
    assert 0 < int(k[0].sum()) < R.G_N and 0 < int((q[1] == 1).sum()) < R.G_N


@pytest.mark.parametrize("name", R.G_CONFIGS)
def test_statements_reproduce_the_reference(golden, name):
    """The formulas alone (no editor class): which calls are controlled is read from the golden's record; every self-attention output of the
    reference's editor is reproduced within fp32 rounding."""
    scale = R.G_D ** -0.5
    ctl = golden["controlled." + name]
    maps, n_maps = None, 0
    for step in range(R.G_STEPS):
        maps, n_maps = None, 0
        for layer in range(R.G_LAYERS):
            is_cross, q, k, v = R.call_inputs(golden, step, layer)
            Q, K, V = _bhnd(q), _bhnd(k), _bhnd(v)
            if is_cross:
                if name == "auto":
                    sets = [R.G_AUTO["ref_token_idx"]] * 3 + [R.G_AUTO["cur_token_idx"]]
                    m, _ = R.token_map_ref(Q, K, scale, sets)
                    maps = m if maps is None else maps + m
                    n_maps += 1
                continue
            if not ctl[step, layer]:
                r, _ = R.mutual_ref(Q, K, V, scale, (0, 1, 2, 3))
            elif name == "plain" or (name == "auto" and n_maps == 0):
                r, _ = R.mutual_ref(Q, K, V, scale, (0, 0, 2, 2))
            elif name == "auto":
                kc, _, _ = R.classes_ref(maps[2], 16, 16, R.G_AUTO["thres"])
                qc, _, _ = R.classes_ref(maps[3], 16, 16, R.G_AUTO["thres"])
                qcls = torch.full((4, R.G_N), R.CLS_ANY, dtype=torch.uint8)
                qcls[1] = qc
                qcls[3] = qc
                r, _ = R.mutual_ref(Q, K, V, scale, (0, 0, 2, 2), qcls, kc[None].repeat(4, 1))
            else:
                qcls, kcls = _mask_classes(name)
                r, _ = R.mutual_ref(Q, K, V, scale, (0, 0, 2, 2), qcls, kcls)
            want = torch.from_numpy(golden["out." + name][step, layer // 2]).to(R.F64)
            err = float((_rows_out(r) - want).abs().max())
            assert err < TOL, (name, step, layer, err)


def test_empty_class_is_the_mean_of_v(golden):
    """the reference's sim + finfo.min on every key: the golden's foreground queries of `mask_empty` equal the plain mean of the source's V"""
    qcls, _ = _mask_classes("mask_empty")
    rows = [i for i, r in enumerate(R.G_ROWS) if int(qcls[1, r]) == 1]
    assert rows
    V = _bhnd(golden["v_self"])
    mean = V.mean(2)                                                    # [B, H, D]
    got = torch.from_numpy(golden["out.mask_empty"][1, 1]).to(R.F64)    # step 1, block 1: controlled
    for b, s in ((1, 0), (3, 2)):
        want = mean[s].reshape(-1)
        assert float((got[b][rows] - want[None]).abs().max()) < 1e-6


class _Attn:
    heads, dim_head, scale = R.G_H, R.G_D, R.G_D ** -0.5


def _packed(q, k, v):
    """(b h) n d operands -> the packed [B n, 3 inner] projection CrossAttention.rows hands to an editor"""
    def rows(t):
        return t.reshape(R.G_B, R.G_H, t.shape[1], R.G_D).permute(0, 2, 1, 3).reshape(R.G_B * t.shape[1], R.G_H * R.G_D)
    return torch.cat([rows(q), rows(k), rows(v)], 1).contiguous()


def _editor(name):
    import anyedit_amd.masactrl as M
    kw = dict(start_step=R.G_START_STEP, start_layer=R.G_START_LAYER, total_steps=R.G_STEPS)
    if name == "base":
        return M.AttentionBase()
    if name == "plain":
        return M.MutualSelfAttentionControl(**kw)
    if name == "auto":
        return M.MutualSelfAttentionControlMaskAuto(**kw, **R.G_AUTO)
    ms, mt = R.golden_masks(name)
    return M.MutualSelfAttentionControlMask(**kw, mask_s=ms, mask_t=mt)


@pytest.mark.parametrize("name", R.G_CONFIGS)
def test_editors_count_gate_and_compute_like_the_reference(golden, name, monkeypatch):
    """The editor classes driven through the calls of two denoising steps, the operators they launch replaced by the float64 statements on the
    same strided operands: the same counting, the same calls taken over (the golden's record), the same outputs — and the launches asked for:
    one stride-only `attention` for plain control, ONE `attention_mutual` for all four branches of a masked call."""
    from anyedit_amd import ops
    fake = R.cpu_ops()
    fake.install(monkeypatch, ops)
    ed = _editor(name)
    ed.num_att_layers = R.G_LAYERS
    ctl = golden["controlled." + name]
    inner = R.G_H * R.G_D
    taken = []
    for step in range(R.G_STEPS):
        for layer in range(R.G_LAYERS):
            assert (ed.cur_step, ed.cur_att_layer) == (step, layer)
            is_cross, q, k, v = R.call_inputs(golden, step, layer)
            before = len(fake.calls)
            if is_cross:
                qr = _packed(q, q, q)[:, :inner].contiguous()
                kv = _packed(k, k, v)[:, inner:].contiguous()
                s_q, s_k = (R.G_N * inner, R.G_D, inner), (R.G_NK * 2 * inner, R.G_D, 2 * inner)
                o = ed(_Attn, True, R.G_B, R.G_N, lambda: fake.attention(qr, kv, kv[:, inner:], R.G_B, R.G_H, R.G_N, R.G_NK, R.G_D, _Attn.scale, s_q, s_k, s_k),
                       q=qr, kv=kv, Nk=R.G_NK)
                assert ("attention", R.G_B, R.G_N, R.G_NK) in fake.calls[before:]      # a cross-attention is never taken over
                continue
            qkv = _packed(q, k, v)
            s = (R.G_N * 3 * inner, R.G_D, 3 * inner)
            o = ed(_Attn, False, R.G_B, R.G_N, lambda: fake.attention(qkv, qkv[:, inner:], qkv[:, 2 * inner:], R.G_B, R.G_H, R.G_N, R.G_N, R.G_D, _Attn.scale, s, s, s),
                   qkv=qkv)
            new = [c for c in fake.calls[before:] if c[0] in ("attention", "attention_mutual")]
            assert len(new) == 1, new                                                  # one attention launch per call, controlled or not
            was_ctl = new[0] != ("attention", R.G_B, R.G_N, R.G_N)
            assert was_ctl == bool(ctl[step, layer]), (name, step, layer, new)
            if was_ctl:
                taken.append((step, layer))
                if name.startswith("mask") or name == "auto":
                    assert new[0] == ("attention_mutual", R.G_B, R.G_N, (0, 0, 2, 2))
                else:
                    assert new[0] == ("attention", 2, 2 * R.G_N, R.G_N)
            want = torch.from_numpy(golden["out." + name][step, layer // 2]).to(R.F64)
            err = float((o.reshape(R.G_B, R.G_N, inner)[:, list(R.G_ROWS)].to(R.F64) - want).abs().max())
            assert err < TOL, (name, step, layer, err)
    assert (ed.cur_step, ed.cur_att_layer) == (R.G_STEPS, 0)
    if name != "base":
        assert ed.controlled == taken and taken == [(1, 2), (1, 4)]
    ed.reset()
    assert (ed.cur_step, ed.cur_att_layer) == (0, 0)


def test_auto_margin_of_the_golden(golden):
    assert float(golden["auto_margin"]) >= 1e-4


def test_mask_validation():
    import anyedit_amd.masactrl as M
    ok = torch.zeros(8, 8)
    ok[2:5, 3:6] = 1
    M.MutualSelfAttentionControlMask(mask_s=ok, mask_t=ok)
    M.MutualSelfAttentionControlMask()
    bad = ok.clone()
    bad[0, 0] = 0.5
    with pytest.raises(ValueError, match="only 0 and 1"):
        M.MutualSelfAttentionControlMask(mask_s=bad, mask_t=ok)
    with pytest.raises(ValueError, match="only 0 and 1"):
        M.MutualSelfAttentionControlMask(mask_s=ok, mask_t=bad * 2)
    with pytest.raises(ValueError, match="or neither"):
        M.MutualSelfAttentionControlMask(mask_s=ok)
    with pytest.raises(ValueError, match="or neither"):
        M.MutualSelfAttentionControlMask(mask_t=ok)
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        M.MutualSelfAttentionControlMask(mask_s=ok[None], mask_t=ok)
    ed = M.MutualSelfAttentionControlMask(start_step=0, start_layer=0, mask_s=ok, mask_t=ok)
    ed.num_att_layers = 2
    with pytest.raises(ValueError, match="two samples per half"):
        ed(_Attn, False, 6, 64, lambda: None, qkv=torch.zeros(6 * 64, 48))


def test_registration_on_the_sd15_layout():
    """SD-1.5's block layout (channel_mult 1-2-4-4, two ResBlocks per level, transformers at the three upper levels) at a narrow width: 16
    transformer blocks = 32 CrossAttention modules, as the reference counts them (masactrl_utils.py:204-212)."""
    import anyedit_amd.masactrl as M
    from anyedit_amd.ldm.modules.attention import CrossAttention
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    unet = UNetModel(image_size=32, in_channels=4, model_channels=32, out_channels=4, num_res_blocks=2, attention_resolutions=[4, 2, 1],
                     channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=16, legacy=False,
                     use_checkpoint=False)
    model = types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet))
    mods = [m for m in unet.modules() if isinstance(m, CrossAttention)]
    assert all("editor" not in m.__dict__ for m in mods)
    ed = M.MutualSelfAttentionControl()
    assert M.regiter_attention_editor_ldm is M.register_attention_editor_ldm
    M.regiter_attention_editor_ldm(model, ed)
    assert ed.num_att_layers == 32 and len(mods) == 32
    assert all(m.__dict__.get("editor") is ed for m in mods)
    assert M.unregister(model) == 32
    assert sum("editor" in m.__dict__ for m in mods) == 0
    assert M.unregister(model) == 0


def test_c_abi_is_declared_and_bound():
    from anyedit_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "anyedit_hip.h")).read()
    for name in ("ae_attn_mutual_bf16", "ae_attn_token_map_bf16", "ae_masactrl_classes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"


@pytest.mark.parametrize("case", R.CLASS_CASES, ids=[c[0] for c in R.CLASS_CASES])
def test_class_cases_keep_clear_of_the_threshold(case):
    """The GPU suite excuses pixels whose float64 normalised value lies within CLS_BOUND of the threshold, at most 1 % of a case: the seeds are
    chosen so that the statement's own count stays under that (here: none at all, except the pixel that meets the threshold on purpose)."""
    _, S, R_, thres, kind, seed = case
    maps = R.class_case_maps(S, kind, seed)
    for i in range(maps.shape[0]):
        cls, counts, norm = R.classes_ref(maps[i], S, R_, thres)
        assert int(counts.sum()) == R_ * R_ and int(counts[1]) == int(cls.sum())
        if kind == "constant" and i == 1:
            assert int(cls.sum()) == 0
            continue
        near = int(((norm - thres).abs() <= R.CLS_BOUND).sum())
        if kind == "exact" and i == 1:
            hit = norm == thres
            assert int(hit.sum()) >= 1 and bool((cls[hit] == 1).all())    # >= : the threshold itself is class 1
            assert near == int(hit.sum())                                 # and nothing else is near
        else:
            assert near <= 0.01 * R_ * R_ and near == 0, (case, near)
        assert 0 < int(cls.sum()) < R_ * R_


def test_nearest_index_is_interpolates():
    for S, R_ in ((4, 4), (4, 8), (16, 16), (16, 32), (16, 64), (16, 24), (32, 16), (5, 13)):
        x = torch.arange(S, dtype=torch.float32)[None, None, None, :].repeat(1, 1, 1, 1)
        want = F.interpolate(x, (1, R_)).flatten().long().numpy()
        assert np.array_equal(R.nearest_index(R_, S), want), (S, R_)
