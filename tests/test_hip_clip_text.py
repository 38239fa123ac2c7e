"""GPU tests of the CLIP text tower: the causal attention kernel against float64, causality as a property, the tiny tower against the
transformers golden and the full-size tower against the restatement (both under the project's 1.5 x control rule), graph capture without
allocations, and `edit_text` end to end.  Every case runs once."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import clip_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0x7FA5          # a NaN bit pattern no kernel writes
TINY = dict(vocab_size=256, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
            eos_token_id=255, pad_token_id=255, bos_token_id=254)


def _tiny(act="quick_gelu", **kw):
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    g = load_golden("clip_text_tiny")
    sd = sub_sd(g, "w.")
    m = FrozenCLIPEmbedder(config=dict(TINY, hidden_act=act), **kw)
    m.load_state_dict(sd)
    return m.to(DEV), sd, g


# ------------------------------------------------------------------------------------------------------------ the attention kernel
@pytest.mark.parametrize("BH", [(1, 1), (2, 12), (12, 12)], ids=lambda v: f"BH{v[0] * v[1]}")
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 64, 77, 96, 128])
def test_causal_attention_vs_float64(N, D, BH):
    """Every element of every row against float64 on the bf16 inputs, with the bound tools/route_check.py applies to attention outputs:
    |got - ref| <= 2^-8 |ref| + 2^-8 (P @ |V|), P the float64 probabilities (output rounding + bf16 probabilities in the PV product).
    The output sits between sentinel guards and a second launch repeats it bit for bit."""
    from anyedit_amd import ops
    B, H = BH
    C = H * D
    gen = torch.Generator().manual_seed(1000 * N + 10 * D + B * H)
    qkv = torch.randn(B * N, 3 * C, generator=gen).to(BF)          # q, k ~ N(0, 1), logits scaled by D^-0.5: unit-variance logits
    dq = qkv.to(DEV)
    st = (N * 3 * C, D, 3 * C)
    total, guard = B * N * C, 4096
    bits = []
    for _ in range(2):
        buf = torch.empty(total + 2 * guard, dtype=BF, device=DEV)
        buf.view(torch.int16).fill_(SENT)
        out = buf[guard:guard + total].view(B, N, C)
        ops.attention_causal_short(dq, dq[:, C:], dq[:, 2 * C:], B, H, N, D, D ** -0.5, st, st, st, out=out)
        torch.cuda.synchronize()
        iv = buf.view(torch.int16)
        assert bool((iv[:guard] == SENT).all()) and bool((iv[guard + total:] == SENT).all()), "wrote outside its output"
        bits.append(out.clone().view(torch.int16).cpu())
    assert torch.equal(bits[0], bits[1]), "two launches differ"
    got = bits[0].view(BF).to(F64).view(B, N, H, D).transpose(1, 2)
    assert torch.isfinite(got).all()
    x = qkv.to(F64).view(B, N, 3, H, D)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))       # [B, H, N, D]
    logits = (q @ k.transpose(-1, -2)) * D ** -0.5
    logits = logits.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    P = logits.softmax(-1)
    ref = P @ v
    bnd = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * (P @ v.abs()) + 1e-30
    ratio = float(((got - ref).abs() / bnd).max())
    print(f"causal attention N={N} D={D} B*H={B * H}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(got[:, :, 0], v[:, :, 0]), "row 0 has one live key: it must return v[0] exactly"


def test_attention_wrapper_refusals_on_gpu():
    from anyedit_amd import ops, _lib
    x = torch.zeros(129, 192, dtype=BF, device=DEV)
    with pytest.raises(_lib.AnyEditHipError, match="sequence length 129"):
        ops.attention_causal_short(x, x[:, 64:], x[:, 128:], 1, 1, 129, 64, 0.125, (129 * 192, 64, 192), (129 * 192, 64, 192), (129 * 192, 64, 192))
    x = torch.zeros(8, 120, dtype=BF, device=DEV)
    with pytest.raises(_lib.AnyEditHipError, match="head_dim 40"):
        ops.attention_causal_short(x, x[:, 40:], x[:, 80:], 1, 1, 8, 40, 0.125, (8 * 120, 40, 120), (8 * 120, 40, 120), (8 * 120, 40, 120))


# ------------------------------------------------------------------------------------------------------------ small kernels
def test_embed_clamps_device_ids_and_bias_act_matches_float64():
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(3)
    tok, pos = torch.randn(50, 64, generator=gen).to(BF), torch.randn(77, 64, generator=gen).to(BF)
    for dt in (torch.int32, torch.int64):
        ids = torch.tensor([[0, 49, 50, -3, 7], [1, 2, 3, 1000000, 4]], dtype=dt)
        got = ops.clip_embed(ids.to(DEV), tok.to(DEV), pos.to(DEV)).float().cpu()
        ref = (tok.float()[ids.long().clamp(0, 49)] + pos.float()[:5]).to(BF).float().reshape(10, 64)
        assert torch.equal(got, ref)                                # out-of-range ids land on the table's edge rows, never outside
    u = torch.randn(37, 512, generator=gen) * 3
    b = torch.randn(512, generator=gen)
    for act, fn in ((ops.ACT_QUICK_GELU, lambda t: t * torch.sigmoid(1.702 * t)), (ops.ACT_GELU, torch.nn.functional.gelu)):
        got = ops.bias_act(u.to(DEV), b.to(DEV), act).to(F64).cpu()
        ref = fn((u + b).to(F64))
        # one bf16 rounding of the result (2^-9 relative) + the fast sigmoid / erf (1.5e-7 absolute on erf, 1 ulp rcp / exp2)
        assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6 * (u + b).abs().to(F64) + 1e-30).all()), act
    z = torch.randn(3 * 5, 64, generator=gen).to(BF)
    ids = torch.tensor([[9, 7, 1, 7, 7], [1, 1, 1, 1, 7], [1, 2, 3, 4, 5]])
    got = ops.clip_pool_eos(ids.to(DEV), z.to(DEV), 7).cpu()
    assert torch.equal(got, torch.stack([z[1], z[5 + 4], z[10]]))       # first EOS; row 0 when there is none


# ------------------------------------------------------------------------------------------------------------ causality
@pytest.mark.parametrize("j", [1, 38, 76])
def test_causality_is_a_property_of_every_layer(j):
    """Changing the token at position j leaves rows < j of every layer's output bit-identical and changes row j — what fails if the mask is
    off by one or a key fragment above the diagonal is read."""
    m, sd, g = _tiny()
    ids = T(g["input_ids"])[2:3].clone()                           # the row without padding
    ids2 = ids.clone()
    ids2[0, j] = (int(ids[0, j]) + 17) % 250
    outs = []
    with torch.no_grad():
        for x in (ids, ids2):
            o = m.transformer(x, output_hidden_states=True)
            outs.append([h.clone().cpu() for h in o.hidden_states] + [o.last_hidden_state.clone().cpu()])
    assert len(outs[0]) == TINY["num_hidden_layers"] + 2
    for li, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a[0, :j], b[0, :j]), f"layer output {li}: a row before position {j} changed"
        assert not torch.equal(a[0, j], b[0, j]), f"layer output {li}: row {j} did not change"


# ------------------------------------------------------------------------------------------------------------ tiny tower vs golden
def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_tiny_tower_vs_transformers_golden(act):
    """Every stored output of the fixture: err(HIP) <= 1.5 x err(control), control = clip_ref(bf16_storage=True) on the same weights."""
    m, sd, g = _tiny(act)
    o = load_golden("clip_text_tiny_" + act)
    ids = T(g["input_ids"])
    L = TINY["num_hidden_layers"]
    ctl = clip_ref.clip_text_forward(sd, ids, 2, act=act, eos_token_id=255, bf16_storage=True)
    report, ok = [], True
    with torch.no_grad():
        m.layer = "last"
        ok &= _judge("last_hidden_state", m.encode_ids(ids), ctl["last_hidden_state"], T(o["last_hidden_state"]), report)
        m.layer = "pooled"
        p = m.encode_ids(ids)
        assert p.shape == (4, 1, TINY["hidden_size"])
        ok &= _judge("pooler_output", p[:, 0], ctl["pooler_output"], T(o["pooler_output"]), report)
        m.layer = "hidden"
        for idx in list(range(L + 1)) + [-1, -2]:
            m.layer_idx = idx
            ok &= _judge(f"hidden_states[{idx}]", m.encode_ids(ids), ctl["hidden_states"][idx], T(o[f"hidden_states.{idx % (L + 1)}"]), report)
        out = m.transformer(ids.to(DEV), output_hidden_states=True)          # the transformers-style call, ids already on the device
        ok &= _judge("transformer().last_hidden_state", out[0], ctl["last_hidden_state"], T(o["last_hidden_state"]), report)
        assert len(out.hidden_states) == L + 1 and out.pooler_output.shape == (4, TINY["hidden_size"])
    print("\n".join(report))
    assert ok, "\n".join(report)


class _StubTokenizer:
    pad_token_id, eos_token_id, bos_token_id = 255, 255, 254

    def __init__(self, raw):
        self.raw = raw

    def __call__(self, text, padding=None, **kw):
        if padding == "max_length":      # FrozenCLIPEmbedder.forward's call: BOS + tokens + EOS, truncated / padded to 77
            rows = [([254] + list(r)[:75] + [255] + [255] * 77)[:77] for r in self.raw]
            return {"input_ids": torch.tensor(rows)}
        return {"input_ids": [list(r) for r in self.raw]}


@pytest.mark.parametrize("clip_skip", [0, 2])
def test_hacked_long_prompt_forward_vs_reference_golden(clip_skip, monkeypatch):
    from anyedit_amd.cldm import hack
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    monkeypatch.setattr(FrozenCLIPEmbedder, "forward", FrozenCLIPEmbedder.forward)
    monkeypatch.setattr(FrozenCLIPEmbedder, "clip_skip", 0, raising=False)
    g = load_golden("clip_text_tiny")
    raw = [g[f"raw.{i}"].tolist() for i in range(4)]
    m, sd, _ = _tiny(tokenizer=_StubTokenizer(raw))
    hack.hack_everything(clip_skip=clip_skip)
    z = T(load_golden(f"clip_text_tiny_hack{clip_skip}")["z"])
    with torch.no_grad():
        got = m(["a", "b", "c", "d"])
    assert got.shape == (4, 231, TINY["hidden_size"])
    ctl = clip_ref.hacked_forward(sd, T(g["framed"]), 2, clip_skip=clip_skip, bf16_storage=True)
    report = []
    ok = _judge(f"hacked forward clip_skip={clip_skip}", got, ctl, z, report)
    print(report[0])
    assert ok, report[0]
    with pytest.raises(ValueError, match="clip_skip"):
        hack.encode_framed(m, g["framed"], clip_skip=9)


# ------------------------------------------------------------------------------------------------------------ full size
def _vitl():
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder, CLIP_VIT_L_TEXT
    sd = clip_ref.seeded_state_dict(CLIP_VIT_L_TEXT, seed=0)
    with torch.device("meta"):
        m = FrozenCLIPEmbedder()
    m.load_state_dict(sd, assign=True)
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 49406, (3, 77), generator=gen)
    ids[:, 0] = 49406
    for b, n in enumerate((9, 40, 76)):
        ids[b, n:] = 49407
    return m.to(DEV), sd, ids


def test_full_size_tower_vs_restatement():
    """ViT-L/14 text geometry, seeded weights, B = 3, EOS at 9 / 40 / 76: HIP vs clip_ref fp32 under the 1.5 x control rule (the control's own
    rel-L2 at this geometry: 8.0e-3 on a CPU run with this seed)."""
    m, sd, ids = _vitl()
    ref = clip_ref.clip_text_forward(sd, ids, 12, eos_token_id=49407)
    ctl = clip_ref.clip_text_forward(sd, ids, 12, eos_token_id=49407, bf16_storage=True)
    report, ok = [], True
    with torch.no_grad():
        ok &= _judge("ViT-L last_hidden_state", m.encode_ids(ids), ctl["last_hidden_state"], ref["last_hidden_state"], report)
        m.layer = "pooled"
        ok &= _judge("ViT-L pooler_output", m.encode_ids(ids)[:, 0], ctl["pooler_output"], ref["pooler_output"], report)
        m.layer, m.layer_idx = "hidden", -2
        ok &= _judge("ViT-L hidden_states[-2]", m.encode_ids(ids), ctl["hidden_states"][-2], ref["hidden_states"][-2], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ graph, allocations
def test_encode_is_capturable_and_allocates_nothing_after_the_first_call():
    m, sd, g = _tiny()
    ids = T(g["input_ids"])
    with torch.no_grad():
        first = m.encode_ids(ids).clone()
        m.encode_ids(ids)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        third = m.encode_ids(ids)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        assert after == before, f"{after - before} allocations in the third encode"
        assert torch.equal(third, first)
        # capture on ids that live on the device (no host copy inside the graph), replay after new ids were copied into that buffer
        static_ids = ids.to(DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.encode_ids(static_ids)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.encode_ids(static_ids)
        new_ids = ids.flip(0).contiguous()
        static_ids.copy_(new_ids.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        eager = m.encode_ids(new_ids).clone()
    assert torch.equal(replayed, eager), "graph replay differs from the eager encode of the same ids"
    assert not torch.equal(replayed, first)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_edit_text_equals_edit_on_encoded_ids_and_reads_the_instruction():
    from util_models import TINY_UNET, unzero, randomize_norm_affine, G
    from anyedit_amd.anysd.model import MoE
    from anyedit_amd.anysd.pipeline import EditPipeline
    from anyedit_amd.ldm.models.diffusion.ddpm import DDPM
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    cfg = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
               eos_token_id=255, pad_token_id=255, bos_token_id=254)
    torch.manual_seed(7)
    unet = UNetModel(**dict(TINY_UNET, context_dim=64))
    unzero(unet, G(7), std=0.05)
    randomize_norm_affine(unet, G(8))
    moe = MoE(unet.eval(), expert_num=11, n_tasks=6, context_dim=64, clip_dim=32, ip_tokens=4).eval().requires_grad_(False).to(DEV)
    gen = torch.Generator().manual_seed(9)
    raw = [torch.randint(0, 250, (n,), generator=gen).tolist() for n in (6, 30)]
    te = FrozenCLIPEmbedder(config=cfg, tokenizer=_StubTokenizer(raw))
    te.load_state_dict(clip_ref.seeded_state_dict(cfg, seed=3))
    te = te.to(DEV)
    sched = DDPM(moe.unet, timesteps=1000, linear_start=0.00085, linear_end=0.0120).to(DEV)
    B = 2
    x_T = torch.randn(B, 4, 8, 8, generator=gen).to(DEV)
    img_lat = (torch.randn(B, 4, 8, 8, generator=gen) * 0.18215).to(DEV)
    ref_emb = torch.randn(B, 9, 32, generator=gen).to(DEV)
    code = torch.tensor([1, 3]).to(DEV)
    pipe = EditPipeline(moe, sched, use_graph=True, text_encoder=te)
    ids = _StubTokenizer(raw)(["a", "b"], padding="max_length")["input_ids"]
    from_text = pipe.edit_text(x_T, img_lat, ["a", "b"], ref_emb, code, steps=4).clone()
    from_ids = pipe.edit_text(x_T, img_lat, ids, ref_emb, code, steps=4).clone()
    null_ids = [[254, 255] + [255] * 75]
    null = te.encode_ids(null_ids).clone()
    assert torch.equal(pipe.null_prompt_ehs(), null) and pipe.null_prompt_ehs() is pipe.null_prompt_ehs()      # encoded once, cached
    ehs = te.encode_ids(ids).clone()
    assert ehs.shape == (B, 77, 64)
    plain = pipe.edit(x_T, img_lat, ehs, null, ref_emb, code, steps=4)
    assert torch.isfinite(plain).all()
    assert torch.equal(from_text, plain) and torch.equal(from_ids, plain), "edit_text must equal edit fed the encode_ids output, bit for bit"
    ids2 = ids.clone()
    ids2[0, 3] = (int(ids[0, 3]) + 5) % 250
    other = pipe.edit_text(x_T, img_lat, ids2, ref_emb, code, steps=4)
    assert not torch.equal(other[0], plain[0]), "changing one instruction token must change the latents"
    # the cached empty prompt follows the encoder's weights
    with torch.no_grad():
        te.transformer.text_model.final_layer_norm.bias.add_(0.5)
    assert not torch.equal(pipe.null_prompt_ehs(), null)


def test_trainer_takes_input_ids_when_it_has_a_text_encoder():
    """train.py:644: a batch may carry input_ids; the loss equals the one from the hidden states of those ids, bit for bit."""
    from util_models import TINY_UNET, unzero, randomize_norm_affine, G
    from anyedit_amd.anysd.model import MoE
    from anyedit_amd.anysd.train import AnySDTrainer
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    from oracle import schedule_ref as S
    cfg = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
               eos_token_id=255, pad_token_id=255, bos_token_id=254)
    torch.manual_seed(11)
    unet = UNetModel(**dict(TINY_UNET, context_dim=64))
    unzero(unet, G(11), std=0.05)
    randomize_norm_affine(unet, G(12))
    moe = MoE(unet.eval(), expert_num=11, n_tasks=6, context_dim=64, clip_dim=32, ip_tokens=4).to(DEV)
    te = FrozenCLIPEmbedder(config=cfg)
    te.load_state_dict(clip_ref.seeded_state_dict(cfg, seed=4))
    te = te.to(DEV)
    buffers = S.register_schedule("linear", 1000, 0.00085, 0.0120)
    sa, s1 = (torch.as_tensor(np.asarray(buffers[k])).float().to(DEV) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))
    gen = torch.Generator().manual_seed(13)
    B = 2
    lat, img, noise = (torch.randn(B, 4, 8, 8, generator=gen).to(DEV) for _ in range(3))
    ref_emb = torch.randn(B, 9, 32, generator=gen).to(DEV)
    code, t = torch.tensor([1, 3]).to(DEV), torch.tensor([981, 21]).to(DEV)
    ids = torch.randint(0, 250, (B, 77), generator=gen)
    ids[:, 0], ids[0, 12:], ids[1, 40:] = 254, 255, 255
    tr = AnySDTrainer(moe, sa, s1, text_encoder=te)
    loss_ids, _, _ = tr.forward_loss(lat, img, ids, ref_emb, code, noise, t)
    ehs = te.encode_ids(ids).clone()
    loss_ehs, _, _ = tr.forward_loss(lat, img, ehs, ref_emb, code, noise, t)
    assert torch.isfinite(loss_ids).all() and torch.equal(loss_ids, loss_ehs)
    with pytest.raises(ValueError, match="text_encoder"):
        AnySDTrainer(moe, sa, s1).forward_loss(lat, img, ids, ref_emb, code, noise, t)
