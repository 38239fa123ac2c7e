"""Prompt-to-Prompt on the CPU: the float64 statements of tests/p2p_ref.py and the controller classes of anyedit_amd.prompt2prompt against the
reference's own outputs (tests/golden/p2p.npz, written by tools/gen_golden_p2p.py from the reference's controller classes in fp32).

Tolerance of the pin.  The golden is fp32.  A logit is a sum of D = 8 products scaled once: its absolute error is at most (D + 2) 2^-24 qk with
qk = max scale sum_d |q_d| |k_d| over the call (the magnitude every partial sum is bounded by); a probability e_j / sum e then carries a relative
error of at most 2 (D + 2) 2^-24 qk + 2^-20 (the exponentials' own ulp, the 77- or 289-term sum, the division), which is p2p_ref.eps_prob — the
same expression the GPU suite uses for the kernel's fp32 path.  The mapper product, the blends and the product with V add (2 Nk + 16) 2^-24.  So
    |golden - float64| <= (eps_prob + (2 Nk + 16) 2^-24) sum_j w_j |v_j| + 1e-7,   w_j = |c_j| (P_base |M|)_j + |d_j| P_own,j
per output element (at these operands: 1e-5 .. 1e-4), and the same factor times sum_h w_j, summed over the steps, per store entry.  A wrong gate,
base sample or mapper column moves an output by 1e-1 and more (test_sensitivity_* shows it on the kernel cases)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import p2p_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "p2p.npz")
F64 = torch.float64


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


def _n(name):
    return len(R.G_CONFIGS[name][1])


def _bhnd(t, B):
    return t.reshape(B, R.G_H, t.shape[1], t.shape[2]).to(F64)


def _onehot(mapper):
    M = torch.zeros(mapper.shape[0], 77, 77, dtype=F64)
    for e in range(mapper.shape[0]):
        M[e, mapper[e] % 77, torch.arange(77)] = 1.0
    return M


def _tables(g, name, step):
    """(M [P-1, 77, 77] or None, c, d [P-1, 77]) of the configuration at a step, from the golden's own arrays (the table of the issue)"""
    kind = R.G_CONFIGS[name][0]
    a = torch.from_numpy(g["alpha." + name][step]).to(F64)
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    if kind in ("replace", "replace_blend"):
        M, c0, d0 = torch.from_numpy(g["mapper." + name]).to(F64), one, zero
    elif kind == "refine":
        al = torch.from_numpy(g["alphas." + name]).to(F64)
        M, c0, d0 = _onehot(torch.from_numpy(g["mapper." + name]).long()), al, 1 - al
    elif kind == "reweight":
        M, c0, d0 = None, torch.from_numpy(g["equalizer." + name]).to(F64).expand_as(a), zero
    else:
        al = torch.from_numpy(g["alphas." + name]).to(F64)
        eq = torch.from_numpy(g["equalizer." + name]).to(F64)
        M, c0, d0 = _onehot(torch.from_numpy(g["mapper." + name]).long()), al * eq, (1 - al) * eq
    return M, c0 * a, d0 * a + 1 - a


def _full(P, M, c, d):
    """the tables laid out over the whole [uncond, cond] batch"""
    B = 2 * P
    Mf = None
    if M is not None:
        Mf = torch.zeros(B, 77, 77, dtype=F64)
        Mf[P + 1:] = M
    cf, df = torch.zeros(B, 77, dtype=F64), torch.ones(B, 77, dtype=F64)
    cf[P + 1:], df[P + 1:] = c, d
    return Mf, cf, df


def _self_gate(step, N):
    return step < int(R.G_STEPS * R.G_SELF_REPLACE) and N <= 256


def _tol(Q, K, W, V, D, Nk):
    scale = D ** -0.5
    return (R.eps_prob(D, Nk, R.qk_abs(Q, K, scale)) + (2 * Nk + 16) * 2.0 ** -24)


def _rows_out(r, P, N):
    """[B, H, N, D] -> the conditional half at the golden's rows, [P, rows, H D]"""
    return r.permute(0, 2, 1, 3).reshape(2 * P, N, -1)[P:, R.rows_of(N)]


def _statement_call(g, name, step, layer):
    """float64 output [B, H, N, D], P' and W of one call of a configuration, and the operands"""
    P = _n(name)
    B = 2 * P
    place, is_cross, q, k, v = R.call_inputs(g, step, layer, P)
    Q, K, V = _bhnd(q, B), _bhnd(k, B), _bhnd(v, B)
    scale = R.G_D ** -0.5
    kind = R.G_CONFIGS[name][0]
    if is_cross:
        if kind == "store":
            r, Pp, W = R.p2p_ref(Q, K, V, scale, list(range(B)))
        else:
            Mf, cf, df = _full(P, *_tables(g, name, step))
            r, Pp, W = R.p2p_ref(Q, K, V, scale, R.case_base(B), Mf, cf, df)
    else:
        Pm = torch.softmax(torch.einsum("bhid,bhjd->bhij", Q, K) * scale, -1)
        if kind != "store" and _self_gate(step, Q.shape[2]):
            Pm[P + 1:] = Pm[P]
        r, Pp, W = Pm @ V, Pm, Pm
    return place, is_cross, Q, K, V, r, Pp, W


@pytest.mark.parametrize("name", list(R.G_CONFIGS))
def test_statements_reproduce_the_reference(golden, name):
    """The formulas alone (no controller class): every output of the reference's controller and its final store, within fp32 rounding."""
    P = _n(name)
    store, sbound = {}, {}
    worst = 0.0
    for step in range(R.G_STEPS):
        ci = 0
        for layer in range(len(R.G_LAYERS)):
            place, is_cross, Q, K, V, r, Pp, W = _statement_call(golden, name, step, layer)
            N = Q.shape[2]
            f = _tol(Q, K, W, V, R.G_D, K.shape[2])
            want = torch.from_numpy(golden["out." + name][step, layer][:, :len(R.rows_of(N))]).to(F64)
            bnd = f * _rows_out(W @ V.abs(), P, N) + 1e-7
            ratio = float(((_rows_out(r, P, N) - want).abs() / bnd).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, step, layer, ratio)
            if is_cross:
                store[ci] = store.get(ci, 0) + Pp[P:].sum(1)[:, list(R.G_ROWS)]
                sbound[ci] = sbound.get(ci, 0) + f * W[P:].sum(1)[:, list(R.G_ROWS)] + 1e-7
                ci += 1
    order = [i for place in ("down", "mid", "up") for i, l in enumerate([l for l in R.G_LAYERS if l[1]]) if l[0] == place]
    for slot, ci in enumerate(order):
        want = torch.from_numpy(golden["store." + name][slot]).to(F64)
        ratio = float(((store[ci] - want).abs() / sbound[ci]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, "store", slot, ratio)
    print(f"{name}: worst |statement - golden| / bound {worst:.3f}")


def test_post_edit_store_is_what_the_reference_keeps(golden):
    """the golden decides: the stored maps of an edit configuration are the edited ones — the pre-edit sum misses the golden by far"""
    name, P = "reweight", 2
    pre = 0
    for step in range(R.G_STEPS):
        _, _, Q, K, V, _, _, _ = _statement_call(golden, name, step, 1)
        pre = pre + torch.softmax(torch.einsum("bhid,bhjd->bhij", Q, K) * R.G_D ** -0.5, -1)[P:].sum(1)[:, list(R.G_ROWS)]
    want = torch.from_numpy(golden["store." + name][0]).to(F64)
    assert float((pre - want).abs().max()) > 1e-2


def test_mappers_and_alpha_tables_equal_the_reference(golden):
    from anyedit_amd.prompt2prompt import seq_aligner, ptp_utils
    tok = R.ToyTokenizer()
    for name, (kind, prompts, word) in R.G_CONFIGS.items():
        if kind == "store":
            continue
        alpha = ptp_utils.get_time_words_attention_alpha(prompts, R.G_STEPS, R.cross_steps(word), tok)
        assert tuple(alpha.shape) == (R.G_STEPS + 1, len(prompts) - 1, 1, 1, 77)
        assert np.array_equal(alpha.reshape(R.G_STEPS + 1, -1, 77).numpy(), golden["alpha." + name]), name
        if kind in ("replace", "replace_blend"):
            assert np.array_equal(seq_aligner.get_replacement_mapper(prompts, tok).numpy(), golden["mapper." + name]), name
        if kind in ("refine", "reweight_refine"):
            mp, al = seq_aligner.get_refinement_mapper(prompts, tok)
            assert mp.dtype == torch.int64 and np.array_equal(mp.numpy(), golden["mapper." + name]), name
            assert np.array_equal(al.numpy(), golden["alphas." + name]), name
    sp = golden["mapper.replace_split"][0]
    assert sp[2, 2] == 0.5 and sp[2, 3] == 0.5                                  # "cat" -> the two pieces of "giraffe"
    assert sp[3].sum() == 0 and sp[4, 4] == 1.0                                 # (the reference continues with mapper[j, j]: row 3 stays empty)
    assert (golden["mapper.refine"][0] == -1).sum() == 1                        # the inserted word
    assert (golden["equalizer.reweight"] < 0).sum() == 1                        # one negative value
    assert np.array_equal(ptp_utils.get_word_inds("a giraffe sits", "giraffe", tok), np.array([2, 3]))
    with pytest.raises(ValueError, match="same length"):
        seq_aligner.get_replacement_mapper(["a cat", "a big cat"], tok)


class _Attn:
    heads, dim_head, scale = R.G_H, R.G_D, R.G_D ** -0.5


def _rows2(t, B):
    """(b h) n d -> [B n, h d] float64"""
    return t.reshape(B, R.G_H, t.shape[1], R.G_D).permute(0, 2, 1, 3).reshape(B * t.shape[1], R.G_H * R.G_D).to(F64)


@pytest.mark.parametrize("name", list(R.G_CONFIGS))
def test_controllers_count_gate_and_compute_like_the_reference(golden, name, monkeypatch):
    """The controller classes driven through the calls of four steps by the registration's adapter, the operators they launch replaced by the
    float64 statements on the same strided operands: the reference's outputs, store, blended latents and mask, its counting — and the launches
    asked for.  The expected gates are written down here from the protocol's constants; a gate that never opens (or never closes) fails."""
    import anyedit_amd.prompt2prompt as PP
    from anyedit_amd import ops
    fake = R.cpu_ops()
    fake.install(monkeypatch, ops)
    tok = R.ToyTokenizer()
    kind, prompts, word = R.G_CONFIGS[name]
    P = len(prompts)
    B = 2 * P
    ctl = R.make_controller(name, PP, tok)
    ctl.num_att_layers = len(R.G_LAYERS)
    inner = R.G_H * R.G_D
    expect, worst, sbound = [], 0.0, {}
    for step in range(R.G_STEPS):
        ci = 0
        for layer in range(len(R.G_LAYERS)):
            assert (ctl.cur_step, ctl.cur_att_layer) == (step, layer)
            place, is_cross, q, k, v = R.call_inputs(golden, step, layer, P)
            N, Nk = q.shape[1], k.shape[1]
            ed = PP.ptp_utils._PlacedEditor(ctl, place)
            before = len(fake.calls)
            if is_cross:
                qr, kv = _rows2(q, B), torch.cat([_rows2(k, B), _rows2(v, B)], 1).contiguous()
                s_q, s_k = (N * inner, R.G_D, inner), (Nk * 2 * inner, R.G_D, 2 * inner)
                o = ed(_Attn, True, B, N, lambda: fake.attention(qr, kv, kv[:, inner:], B, R.G_H, N, Nk, R.G_D, _Attn.scale, s_q, s_k, s_k), q=qr, kv=kv, Nk=Nk)
                new = fake.calls[before:]
                acc = step > 0
                # `refine`: the key word is the inserted token, whose alphas is 0, so once the default gate has closed (step 2) c = 0 and d = 1
                # everywhere: the call is the store-only launch and core().  Every other edit configuration keeps its key word's gate open.
                live = kind != "store" and (kind != "refine" or step < int(R.G_STEPS * 0.5))
                if not live:
                    assert new == [("attention_p2p", P, N, Nk, tuple(range(P)), False, acc), ("attention", B, N, Nk)], new
                else:
                    expect.append((step, layer, "cross"))
                    assert new == [("attention_p2p", P, N, Nk, (0,) * P, True, acc), ("attention", P + 1, N, Nk)], new
            else:
                qkv = torch.cat([_rows2(q, B), _rows2(k, B), _rows2(v, B)], 1).contiguous()
                s = (N * 3 * inner, R.G_D, 3 * inner)
                o = ed(_Attn, False, B, N, lambda: fake.attention(qkv, qkv[:, inner:], qkv[:, 2 * inner:], B, R.G_H, N, N, R.G_D, _Attn.scale, s, s, s), qkv=qkv)
                new = fake.calls[before:]
                if kind != "store" and _self_gate(step, N):
                    expect.append((step, layer, "self"))
                    assert new == [("attention", P + 1, N, N), ("attention", P - 1, N, N)], new
                else:
                    assert new == [("attention", B, N, N)], new
            _, _, Q, K, V, _, _, W = _statement_call(golden, name, step, layer)
            want = torch.from_numpy(golden["out." + name][step, layer][:, :len(R.rows_of(N))]).to(F64)
            bnd = _tol(Q, K, W, V, R.G_D, Nk) * _rows_out(W @ V.abs(), P, N) + 1e-7
            if is_cross:
                sbound[ci] = sbound.get(ci, 0) + _tol(Q, K, W, V, R.G_D, Nk) * W[P:].sum(1)[:, list(R.G_ROWS)] + 1e-7
                ci += 1
            got = o.reshape(B, N, inner)[P:, R.rows_of(N)].to(F64)
            ratio = float(((got - want).abs() / bnd).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, step, layer, ratio)
        assert (ctl.cur_step, ctl.cur_att_layer) == (step + 1, 0)
        if kind == "replace_blend":
            x = R.step_latent(golden, step)
            got = ctl.step_callback(x.clone())
            want = torch.from_numpy(golden["blend." + name][step])
            # the reference forms x0 + mask (x1 - x0) in fp32: where the mask is 1 that is x1 up to two roundings
            assert float((got - want).abs().max()) <= 2.0 ** -22 * float(x.abs().max())
            changed = (got[1] != x[0]).any(0)
            assert 0 < int(changed.sum()) < changed.numel()          # the mask is neither empty nor full
            assert torch.equal(got[0], x[0])
        else:
            x = R.step_latent(golden, step)
            assert ctl.step_callback(x) is x
    if kind != "store":
        assert ctl.controlled == expect
        assert any(k == "self" for _, _, k in expect) and not all((s, l, "self") in expect for s in range(R.G_STEPS) for l in (0, 8))
    # the store: 8 cross calls, head sums over the steps, in call order per place
    slot = 0
    order = [i for place in ("down", "mid", "up") for i, l in enumerate([l for l in R.G_LAYERS if l[1]]) if l[0] == place]
    for place, count in (("down", 4), ("mid", 1), ("up", 3)):
        bufs = ctl.attention_store[f"{place}_cross"]
        assert len(bufs) == count and ctl.store_heads[f"{place}_cross"] == [R.G_H] * count
        for buf in bufs:
            assert buf.dtype == torch.float32 and tuple(buf.shape) == (P, 256, 77)
            want = torch.from_numpy(golden["store." + name][slot]).to(F64)
            bnd = sbound[order[slot]] + 2.0 ** -22 * want.abs()                  # + the fp32 buffer's own roundings, one per step
            ratio = float(((buf[:, list(R.G_ROWS)].to(F64) - want).abs() / bnd).max())
            assert ratio <= 1.0, (name, slot, ratio)
            slot += 1
    assert all(len(ctl.attention_store[k]) == 0 for k in ("down_self", "mid_self", "up_self"))
    if kind == "store":
        got = np.array(PP.mask_from_CA(ctl, 16, ("up", "down"), prompts, R.G_MASK_WORDS, tokenizer=tok))
        want = golden["mask.store"]
        assert got.shape == want.shape and got.dtype == want.dtype
        differing = int((got != want).sum())
        print(f"mask_from_CA: {int((want > 0).sum())} set, differing {differing}")
        assert 0 < int((want > 0).sum()) < want.size and differing == 0
        avg = ctl.get_average_attention()
        assert float((avg["mid_cross"][0].sum(-1) - 1).abs().max()) < 1e-5   # a mean of probabilities: rows sum to 1
    print(f"{name}: worst |controller - golden| / bound {worst:.3f}")
    ctl.reset()
    assert (ctl.cur_step, ctl.cur_att_layer) == (0, 0) and all(len(v) == 0 for v in ctl.attention_store.values())


def test_three_prompts_with_local_blend_raise(monkeypatch):
    import anyedit_amd.prompt2prompt as PP
    tok = R.ToyTokenizer()
    prompts = R.G_CONFIGS["replace3"][1]
    lb = PP.LocalBlend(prompts, ("cat", "dog", "giraffe"), tokenizer=tok)
    store = {"down_cross": [torch.zeros(3, 256, 77)] * 4, "up_cross": [torch.zeros(3, 256, 77)] * 3}
    with pytest.raises(ValueError, match="exactly two prompts"):
        lb(torch.zeros(3, 4, 16, 16), store)
    with pytest.raises(ValueError, match="tokenizer="):
        PP.LocalBlend(prompts, ("cat", "dog", "giraffe"))
    with pytest.raises(ValueError, match="tokenizer="):
        PP.AttentionReplace(prompts, 4, 0.5, 0.5)


def test_registration_binds_the_place_names():
    import anyedit_amd.prompt2prompt as PP
    from anyedit_amd.ldm.modules.attention import CrossAttention
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    unet = UNetModel(image_size=32, in_channels=4, model_channels=32, out_channels=4, num_res_blocks=2, attention_resolutions=[4, 2, 1],
                     channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=16, legacy=False,
                     use_checkpoint=False)
    model = types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet))
    ctl = PP.AttentionStore()
    assert PP.register_attention_control(model, ctl) is ctl and ctl.num_att_layers == 32
    places = {}
    for m in unet.modules():
        if isinstance(m, CrossAttention):
            ed = m.__dict__["editor"]
            assert ed.controller is ctl
            places[ed.place] = places.get(ed.place, 0) + 1
    assert places == {"down": 12, "mid": 2, "up": 18}
    assert PP.unregister(model) == 32 and PP.unregister(model) == 0
    assert PP.register_attention_control(model, None).num_att_layers == 32 and PP.unregister(model) == 32   # the reference's DummyController


def test_c_abi_is_declared_and_bound():
    from anyedit_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "anyedit_hip.h")).read()
    for name in ("ae_attn_p2p_bf16", "ae_p2p_local_blend_f32"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert f" {name}(" in header, f"{name} is not declared in include/anyedit_hip.h"


# ------------------------------------------------------------------------------------------- what the GPU suite's bounds can tell apart
CASES = R.p2p_cases()


@pytest.mark.parametrize("case", CASES, ids=[R.case_id(c) for c in CASES])
def test_sensitivity_of_the_gpu_bounds(case):
    """Each of four mistakes breaks the GPU test's bound on at least one element of the case's dense variant: the mapper shifted by one token, c
    and d swapped, the sample's own probabilities in place of the base's, the pre-edit store.  With ONE key every softmax is the constant 1, so
    the base's and the sample's probabilities coincide and a 1 x 1 mapper cannot shift: those two are not expected to show at Nk = 1."""
    D, Nk, N, H, B = case
    _, _, _, _, Q, K, V = R.case_operands(case)
    scale = D ** -0.5
    qk = R.qk_abs(Q, K, scale)
    base = R.case_base(B)
    M, c, d = R.case_edit(case, "dense")
    ref, Pp, W = R.p2p_ref(Q, K, V, scale, base, M, c, d)
    bnd = R.p2p_out_bound(ref, W, V, D, Nk, qk)
    sbnd = R.p2p_store_bound(W, Nk, D, qk, H)

    def breaks(M2, c2, d2, base2):
        r2, _, _ = R.p2p_ref(Q, K, V, scale, base2, M2, c2, d2)
        return float(((r2 - ref).abs() / bnd).max())

    figures = {"c and d swapped": breaks(M, d, c, base)}
    if Nk > 1:
        figures["mapper shifted"] = breaks(torch.roll(M, 1, 2), c, d, base)
        own = list(range(B))
        r_own = (R.p2p_ref(Q, K, V, scale, own)[1])                                     # every sample's own probabilities
        Pwrong = Pp.clone()
        for b in range(B // 2 + 1, B):
            Pwrong[b] = (r_own[b] @ M[b].to(F64)) * c[b].to(F64) + r_own[b] * d[b].to(F64)
        figures["own sample as the base"] = float((((Pwrong @ V) - ref).abs() / bnd).max())
    pre = R.p2p_ref(Q, K, V, scale, list(range(B)))[1].sum(1)
    figures["pre-edit store"] = float(((pre - Pp.sum(1)).abs() / sbnd)[B // 2 + 1:].max())
    print(R.case_id(case), {k: f"{v:.1f}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v > 1.0, (k, v)


@pytest.mark.parametrize("case", R.BLEND_CASES, ids=[c[0] for c in R.BLEND_CASES])
def test_blend_cases_keep_clear_of_the_threshold(case):
    """no pixel of the float64 normalised maps lies within blend_band of the threshold — except pixels whose arithmetic is exact in both precisions
    (the `exact` case's multiples of 1/8, and x / x = 1 at the maximum of `at-max`), so the GPU suite asks for the float64 mask outright"""
    _, S, (h, w), L, kind, _ = case
    maps, sets, thr, x = R.blend_case(case)
    out, mask, norm = R.blend_ref(maps, sets, S, thr, x)
    band = R.blend_band(L * max(len(s) for s in sets))
    near = (norm - float(np.float32(thr))).abs() <= band
    if kind == "exact":
        assert int(near.sum()) > 0 and bool((norm[near] == 0.5).all())
    elif kind == "atmax":
        assert int(near.sum()) > 0 and bool((norm[near] == 1.0).all()) and int(mask.sum()) == 0
    else:
        assert int(near.sum()) == 0, (case[0], int(near.sum()))
    if kind == "zero":
        assert bool(torch.isnan(norm[0]).all()) and 0 < int(mask.sum()) < h * w     # sample 0 gives no mask, sample 1 does
    if kind == "empty":
        assert bool(torch.isnan(norm[1]).all())
    if kind == "random":
        assert 0 < int(mask.sum()) < h * w
    assert float(golden_margin()) >= 1e-4


def golden_margin():
    return np.load(GOLDEN)["blend_margin"]


def test_nearest_index_is_interpolates():
    import torch.nn.functional as F
    for S, R_ in ((16, 64), (16, 16), (16, 24), (16, 40), (32, 16)):
        x = torch.arange(S, dtype=torch.float32)[None, None, None, :]
        want = F.interpolate(x, (1, R_)).flatten().long().numpy()
        assert np.array_equal(R.nearest_index(R_, S), want), (S, R_)
