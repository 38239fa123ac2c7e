"""Host-side checks of the CLIP text tower (no GPU): the chain of trust of its fixtures, the checkpoint key schema, the no-network rule, the
chunk framing of the long-prompt forward, the C ABI's argument refusals and the LatentDiffusion / checkpoint wiring."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd, rel_l2, T  # noqa: E402
import clip_ref  # noqa: E402

TINY = dict(vocab_size=256, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
            eos_token_id=255, pad_token_id=255, bos_token_id=254)


def _tiny_embedder(**kw):
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    return FrozenCLIPEmbedder(config=dict(TINY), **kw)


def test_restatement_matches_the_transformers_golden():
    """tests/clip_ref.py (fp32) against what transformers' CLIPTextModel and the reference's _hacked_clip_forward produced: rel-L2 <= 1e-5 on
    every stored tensor (fp32 reassociation noise measured at generation: 4e-7 .. 6e-7)."""
    g = load_golden("clip_text_tiny")
    sd = sub_sd(g, "w.")
    ids = T(g["input_ids"])
    worst = 0.0
    for act in ("quick_gelu", "gelu"):
        o = load_golden("clip_text_tiny_" + act)
        r = clip_ref.clip_text_forward(sd, ids, TINY["num_attention_heads"], act=act, eos_token_id=TINY["eos_token_id"])
        pairs = [("last_hidden_state", r["last_hidden_state"]), ("pooler_output", r["pooler_output"])]
        pairs += [(f"hidden_states.{i}", h) for i, h in enumerate(r["hidden_states"])]
        assert len(r["hidden_states"]) == TINY["num_hidden_layers"] + 1 and f"hidden_states.{len(r['hidden_states'])}" not in o
        for name, got in pairs:
            e = rel_l2(got, T(o[name]))
            worst = max(worst, e)
            assert e <= 1e-5, (act, name, e)
    for skip in (0, 2):
        z = T(load_golden(f"clip_text_tiny_hack{skip}")["z"])
        got = clip_ref.hacked_forward(sd, T(g["framed"]), TINY["num_attention_heads"], clip_skip=skip)
        assert got.shape == z.shape == (4, 231, TINY["hidden_size"])
        e = rel_l2(got, z)
        worst = max(worst, e)
        assert e <= 1e-5, ("hack", skip, e)
    print(f"restatement vs golden: worst rel-L2 {worst:.3e}")
    # the fixture's ids: EOS (the largest id) first appears at 9, 40, 76 (a row without padding) and 1 (the empty prompt)
    assert [(row == TINY["eos_token_id"]).nonzero()[0].item() for row in ids] == [9, 40, 76, 1]
    assert torch.equal(ids.argmax(-1), (ids == TINY["eos_token_id"]).int().argmax(-1))


def test_control_differs_from_fp32_only_by_storage_rounding():
    """The bf16-storage control is the same arithmetic with roundings at the marked points: close to the fp32 restatement, not equal to it."""
    g = load_golden("clip_text_tiny")
    sd, ids = sub_sd(g, "w."), T(g["input_ids"])
    a = clip_ref.clip_text_forward(sd, ids, 2)["last_hidden_state"]
    b = clip_ref.clip_text_forward(sd, ids, 2, bf16_storage=True)["last_hidden_state"]
    e = rel_l2(b, a)
    assert 1e-4 < e < 3e-2, e
    assert torch.equal(b, b.to(torch.bfloat16).float())


def test_key_schema_and_param_count_of_the_default_geometry():
    """ViT-L/14 text: 49408*768 + 77*768 + 12 * (4*(768*768+768) + 2*2*768 + 768*3072+3072 + 3072*768+768) + 2*768 = 123 060 480 in
    2 + 12*16 + 2 = 196 tensors, named as SD-1.5 checkpoints name them below `cond_stage_model.`."""
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    with torch.device("meta"):
        m = FrozenCLIPEmbedder()
    sd = m.state_dict()
    C, I, L = 768, 3072, 12
    want = 49408 * C + 77 * C + L * (4 * (C * C + C) + 2 * 2 * C + C * I + I + I * C + C) + 2 * C
    assert want == 123060480
    assert len(sd) == 196 and sum(v.numel() for v in sd.values()) == want
    p = "transformer.text_model."
    keys = {p + "embeddings.token_embedding.weight", p + "embeddings.position_embedding.weight", p + "final_layer_norm.weight", p + "final_layer_norm.bias"}
    for i in range(L):
        for n in ("layer_norm1", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "layer_norm2", "mlp.fc1", "mlp.fc2"):
            keys |= {f"{p}encoder.layers.{i}.{n}.weight", f"{p}encoder.layers.{i}.{n}.bias"}
    assert set(sd) == keys
    assert sd[p + "encoder.layers.11.mlp.fc1.weight"].shape == (I, C) and sd[p + "embeddings.position_embedding.weight"].shape == (77, C)
    assert all(not v.requires_grad for v in m.parameters()) and not m.transformer.training


def test_position_ids_tolerated_and_fixture_keys_load_strictly():
    g = load_golden("clip_text_tiny")
    sd = sub_sd(g, "w.")
    m = _tiny_embedder()
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd)                                     # strict
    old = dict(sd)
    old["transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    m.load_state_dict(old)                                    # strict, with the buffer old checkpoints carry
    assert torch.equal(m.state_dict()["transformer.text_model.final_layer_norm.bias"], sd["transformer.text_model.final_layer_norm.bias"])
    bad = dict(sd)
    bad["transformer.text_model.embeddings.bogus"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)


def test_packed_weight_images_follow_the_parameters():
    m = _tiny_embedder()
    lay = m.transformer.text_model.encoder.layers[0]
    pk = lay.packed()
    assert lay.packed() is pk and pk.wqkv.shape == (384, 128) and pk.wqkv.dtype == torch.bfloat16 and pk.bqkv.dtype == torch.float32
    assert torch.equal(pk.wqkv[128:256].float(), lay.self_attn.k_proj.weight.detach().to(torch.bfloat16).float())
    tok0 = m.transformer.weights_token()
    sd = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)                                     # a load on the PARENT must reach the layer's cache
    pk2 = lay.packed()
    assert pk2 is not pk and torch.equal(pk2.wqkv[:128].float(), sd["transformer.text_model.encoder.layers.0.self_attn.q_proj.weight"].to(torch.bfloat16).float())
    assert torch.equal(pk2.b1, sd["transformer.text_model.encoder.layers.0.mlp.fc1.bias"])
    assert m.transformer.weights_token() != tok0
    t = m.transformer._tables()
    assert torch.equal(t.tok.float(), sd["transformer.text_model.embeddings.token_embedding.weight"].to(torch.bfloat16).float())


def test_no_network_and_no_tokenizer_is_a_clear_error(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("FrozenCLIPEmbedder tried to open a socket")
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket.socket, "connect_ex", refuse)
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    m = FrozenCLIPEmbedder(version="openai/clip-vit-large-patch14", config=dict(TINY))     # the default hub name: never resolved
    assert m.tokenizer is None and callable(m.encode_ids)
    with pytest.raises(ValueError, match="tokenizer"):
        m.forward("x")
    with pytest.raises(ValueError, match="tokenizer"):
        m.encode("x")


def test_host_ids_are_range_checked_before_any_copy():
    m = _tiny_embedder()
    for bad in ([[254, 256, 255]], torch.tensor([[254, -1, 255]]), np.array([[254, 1000, 255]])):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            m.encode_ids(bad)
    assert m.transformer._ws == {}                            # refused before a workspace (let alone a copy) existed
    with pytest.raises(ValueError, match="position table"):
        m.encode_ids([[1] * 78])
    with pytest.raises(ValueError, match="GPU only"):         # in-range ids on a CPU module: no CPU path
        m.encode_ids([[254, 3, 255]])


def test_geometry_outside_the_kernel_is_refused_at_construction():
    from anyedit_amd.ldm.modules.encoders.modules import CLIPTextTower
    with torch.device("meta"):
        for bad in (dict(hidden_size=80, num_attention_heads=2), dict(max_position_embeddings=129), dict(hidden_act="relu")):
            with pytest.raises(ValueError):
                CLIPTextTower(dict(TINY, **bad))


class _StubTokenizer:
    pad_token_id, eos_token_id, bos_token_id = 255, 255, 254

    def __init__(self, raw):
        self.raw, self.calls = raw, []

    def __call__(self, text, **kw):
        self.calls.append(kw)
        return {"input_ids": [list(r) for r in self.raw]}


def test_hacked_forward_chunking_and_framing(monkeypatch):
    """Host logic of cldm/hack.py:47-60 against the ids the reference's own function fed its transformer (fixture `framed`)."""
    from anyedit_amd.cldm import hack
    g = load_golden("clip_text_tiny")
    raw = [g[f"raw.{i}"].tolist() for i in range(4)]
    assert [len(r) for r in raw] == [5, 75, 76, 200]
    framed = hack.frame_chunks(raw, bos=254, eos=255, pad=255)
    assert np.array_equal(np.asarray(framed), g["framed"])
    f = np.asarray(framed)
    assert f.shape == (4, 3, 77) and (f[:, :, 0] == 254).all()
    assert f[0, 0, 6] == 255 and (f[0, 1, 1:] == 255).all()                  # 5 tokens: EOS at 6, chunks 2 and 3 are [BOS, EOS, PAD...]
    assert f[1, 0, 76] == 255 and f[1, 0, 75] == raw[1][74] and f[1, 1, 1] == 255     # 75 tokens fill chunk 1 exactly
    assert f[2, 1, 1] == raw[2][75] and f[2, 1, 2] == 255                     # the 76th token opens chunk 2
    assert f[3, 2, 1] == raw[3][150] and f[3, 2, 51] == 255 and f[3, 2, 50] == raw[3][199]
    # hack_everything installs the forward on the class; the forward tokenizes without truncation / special tokens and hands on the framed ids
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    monkeypatch.setattr(FrozenCLIPEmbedder, "forward", FrozenCLIPEmbedder.forward)          # restored after the test
    monkeypatch.setattr(FrozenCLIPEmbedder, "clip_skip", 0, raising=False)
    seen = {}
    monkeypatch.setattr(hack, "encode_framed", lambda emb, tokens, clip_skip=0: seen.update(tokens=tokens, skip=clip_skip) or "z")
    hack.hack_everything(clip_skip=2)
    tok = _StubTokenizer(raw)
    m = _tiny_embedder(tokenizer=tok)
    assert m("whatever") == "z" and seen["skip"] == 2 and np.array_equal(np.asarray(seen["tokens"]), g["framed"])
    assert tok.calls == [dict(truncation=False, add_special_tokens=False)]


def test_c_abi_refuses_bad_arguments_before_any_gpu_call():
    from anyedit_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_uint16 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15                    # host memory: every call below must be refused before it is touched
    st = (77 * 384, 64, 384)
    ok_o = (77 * 128, 64, 128)

    def attn(q=p, k=p, v=p, o=p, B=1, H=2, N=77, D=64, qs=st, ks=st, vs=st, os_=ok_o, scale=0.125):
        return L.ae_attn_causal_short_bf16(q, k, v, o, B, H, N, D, *qs, *ks, *vs, *os_, scale, None)

    for kw, msg in ((dict(N=129), b"sequence length 129"), (dict(N=0), b"sequence length 0"), (dict(D=40), b"head_dim 40"), (dict(q=None), b"null pointer"),
                    (dict(o=None), b"null pointer"), (dict(qs=(77 * 384, 64, 380)), b"strides"), (dict(vs=(77 * 384, 60, 384)), b"strides"),
                    (dict(os_=(77 * 128, 64, 126)), b"strides"), (dict(k=p + 2), b"aligned"), (dict(B=0), b"bad sizes"), (dict(scale=0.0), b"scale")):
        assert attn(**kw) == -1 and msg in L.ae_last_error(), (kw, L.ae_last_error())
    e = L.ae_clip_embed_bf16
    assert e(None, 0, p, p, p, 1, 77, 128, 256, 77, None) == -1 and b"null pointer" in L.ae_last_error()
    assert e(p, 0, p, p, p, 1, 78, 128, 256, 77, None) == -1 and b"position table" in L.ae_last_error()
    assert e(p, 0, p, p, p, 1, 77, 100, 256, 77, None) == -1 and b"multiple of 8" in L.ae_last_error()
    assert e(p, 1, p + 8, p, p, 1, 77, 128, 256, 77, None) == -1 and b"aligned" in L.ae_last_error()
    a = L.ae_bias_act_f32_bf16
    assert a(None, 512, p, p, 512, 77, 512, 0, None) == -1 and b"null pointer" in L.ae_last_error()
    assert a(p, 512, p, p, 512, 77, 510, 0, None) == -1 and b"multiple of 4" in L.ae_last_error()
    assert a(p, 256, p, p, 512, 77, 512, 0, None) == -1 and b"row strides" in L.ae_last_error()
    assert a(p, 512, p, p, 512, 77, 512, 2, None) == -1 and b"act must be" in L.ae_last_error()
    q = L.ae_clip_pool_eos_bf16
    assert q(p, 0, None, p, 1, 77, 128, 255, None) == -1 and b"null pointer" in L.ae_last_error()
    assert q(p, 0, p, p, 1, 77, 100, 255, None) == -1 and b"multiple of 8" in L.ae_last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    from anyedit_amd import ops
    x = torch.zeros(77, 384, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.attention_causal_short(x, x[:, 128:], x[:, 256:], 1, 2, 77, 64, 0.125, (77 * 384, 64, 384), (77 * 384, 64, 384), (77 * 384, 64, 384))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.clip_embed(torch.zeros(1, 77, dtype=torch.int64), x, x)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.bias_act(torch.zeros(77, 512), torch.zeros(512))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.clip_pool_eos(torch.zeros(1, 77, dtype=torch.int64), x, 255)


def test_latent_diffusion_cond_stage_wiring():
    from anyedit_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from anyedit_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder

    class Probe(torch.nn.Module):
        def forward(self, x, t, context=None):
            return x

    base = LatentDiffusion(Probe(), conditioning_key="crossattn")
    assert base.cond_stage_model is None and not [k for k in base.state_dict() if k.startswith("cond_stage_model")]
    for cfg in ("__is_unconditional__", "__is_first_stage__", {"target": "torch.nn.Identity"},
                {"target": "ldm.modules.encoders.modules.FrozenOpenCLIPEmbedder"}):
        m = LatentDiffusion(Probe(), conditioning_key="crossattn", cond_stage_config=cfg)
        assert m.cond_stage_model is None and set(m.state_dict()) == set(base.state_dict())
        with pytest.raises(RuntimeError, match="no cond stage"):
            m.get_learned_conditioning(["x"])
    with torch.device("meta"):                                # the default (ViT-L) geometry without its 490 MB: built on the meta device
        big = FrozenCLIPEmbedder()
    m = LatentDiffusion(Probe(), conditioning_key="crossattn", cond_stage_config=big)
    assert m.cond_stage_model is big and len([k for k in m.state_dict() if k.startswith("cond_stage_model.")]) == 196
    m = LatentDiffusion(Probe(), conditioning_key="crossattn",     # the schedule tables are numpy: the LatentDiffusion itself is built on the CPU
                        cond_stage_config={"target": "ldm.modules.encoders.modules.FrozenCLIPEmbedder", "params": {"config": dict(TINY)}})
    assert isinstance(m.cond_stage_model, FrozenCLIPEmbedder) and not m.cond_stage_model.training
    assert all(not p.requires_grad for p in m.cond_stage_model.parameters())
    assert "cond_stage_model.transformer.text_model.embeddings.token_embedding.weight" in m.state_dict()
    called = {}
    m.cond_stage_model.encode = lambda c: called.setdefault("c", c) or "ehs"
    assert m.get_learned_conditioning(["make it red"]) == ["make it red"] and called["c"] == ["make it red"]


def test_full_checkpoint_routes_cond_stage_to_the_tower(tmp_path):
    from anyedit_amd.checkpoints import load_sd_checkpoint, text_encoder_state_dict
    torch.manual_seed(0)
    src = _tiny_embedder()
    own = src.state_dict()
    ck = {"cond_stage_model." + k: torch.randn_like(v) for k, v in own.items()}
    ck["cond_stage_model.transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    ck["model.diffusion_model.time_embed.0.weight"] = torch.zeros(4, 4)
    ck["first_stage_model.encoder.conv_in.weight"] = torch.zeros(4, 4)
    path = tmp_path / "sd15_tiny.ckpt"
    torch.save({"state_dict": ck}, path)
    dst = _tiny_embedder()
    assert load_sd_checkpoint(str(path), text_encoder=dst) == ["text_encoder"]
    for k, v in dst.state_dict().items():
        assert torch.equal(v, ck["cond_stage_model." + k]), k
    # the other layouts of the same tensors: the tower alone, transformers' CLIPTextModel with and without its text_model level
    for strip in ("", "transformer.", "transformer.text_model."):
        alt = {k[len(strip):]: v for k, v in own.items()}
        got = text_encoder_state_dict(dst, alt)
        assert set(got) == set(own) and all(got[k] is own[k] for k in own)
    with pytest.raises(KeyError):
        text_encoder_state_dict(dst, {k: v for k, v in ck.items() if "layers.1.mlp.fc2.bias" not in k})
    bad = dict(ck)
    bad["cond_stage_model.transformer.text_model.final_layer_norm.weight"] = torch.zeros(64)
    with pytest.raises(ValueError, match="shape"):
        text_encoder_state_dict(dst, bad)


def test_pipeline_edit_text_needs_an_encoder_and_keeps_edit_signature():
    import inspect
    from anyedit_amd.anysd.pipeline import EditPipeline
    sig = inspect.signature(EditPipeline.edit)
    assert list(sig.parameters)[:7] == ["self", "x_T", "img_lat", "ehs", "null_ehs", "ref_embeds", "edit_code"]
    assert list(inspect.signature(EditPipeline.prepare).parameters) == ["self", "img_lat", "ehs", "null_ehs", "ref_embeds", "edit_code"]
    assert inspect.signature(EditPipeline.__init__).parameters["text_encoder"].default is None
    pipe = EditPipeline.__new__(EditPipeline)
    pipe.text_encoder = None
    with pytest.raises(ValueError, match="text_encoder"):
        pipe.edit_text(None, None, [[254, 255]], None, None)
