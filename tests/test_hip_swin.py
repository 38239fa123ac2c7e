"""GPU tests of GroundingDINO's Swin backbone: its two kernels against float64 between sentinel guards, both tiny towers against the reference's
golden at every stored image and the Swin-B widths against the restatement (under the project's 1.5 x control rule), the relative position bias
after an in-place change of its table, batch independence, the NestedTensor masks, graph capture without allocations and the wrappers'
refusals.  Every case runs once.

Three comparison rules.  Attention rule (tests/test_hip_clip_text.py, tools/route_check.py): every element within 2^-8 |ref| + 2^-8 (P @ |V|) +
1e-30 of float64, P the float64 probabilities (pad keys included).  Kernel rule: every element within 2^-8 |ref| + 1e-30 of float64 (one bf16
rounding).  Tower rule: err(HIP) <= 1.5 x err(bf16-storage control), both against the stored or fp32 reference."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, rel_l2, T  # noqa: E402
import swin_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0x7FA5          # a NaN bit pattern no kernel writes
GUARD = 4096
TINY = {
    "a": dict(embed_dim=32, depths=[2, 2, 2], num_heads=[1, 2, 4], window_size=7),
    "b": dict(embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=12),
}
SIZES = {"a": [(50, 38)], "b": [(90, 106), (40, 40)]}
CASES = [(g, s) for g in TINY for s in SIZES[g]]
CASE_IDS = [f"{g}_{s[0]}x{s[1]}" for g, s in CASES]
MAPS = {"one": lambda ws: (ws, ws), "pad2x2": lambda ws: (ws + 1, 2 * ws - 1), "small": lambda ws: (3, 5), "regions": lambda ws: (2 * ws + 3, 3 * ws)}


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
    return bits[0]


def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


# ------------------------------------------------------------------------------------------------------------ window attention
def _attn_inputs(ws, nH, B, H, W, gen, q_offset=None):
    C = nH * 32
    qkv = torch.randn(B * H * W, 3 * C, generator=gen)
    if q_offset is not None:
        qkv[:, :C] += q_offset
    qkv = qkv.to(BF)
    qkv_bias = torch.randn(3 * C, generator=gen) * 0.5
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=gen)
    return C, qkv, qkv_bias, R.gathered_bias(table, ws)


def _attn_float64(qkv, qkv_bias, bias, B, H, W, nH, ws, shift, scale):
    """The reference way in float64 from the bf16 inputs: pad with bias rows (rounded to bf16: what the qkv GEMM stores for a zero row), roll,
    partition, + bias table and -100 mask, softmax, reverse, roll back, crop -> (out, P @ |V|) as [B*H*W, C]."""
    C3 = qkv.shape[1]
    Hp, Wp = R.up(H, ws), R.up(W, ws)
    padded = qkv_bias.to(BF).to(F64).expand(B, Hp, Wp, C3).clone()
    padded[:, :H, :W] = qkv.to(F64).view(B, H, W, C3)
    o, pav = R.window_attention(padded, bias.to(F64), H, W, nH, ws, shift, scale)
    return o.reshape(B * H * W, -1), pav.reshape(B * H * W, -1)


def _run_attn(qkv, qkv_bias, bias, B, H, W, nH, ws, shift, scale):
    """The launch on strided buffers (the pad columns of qkv hold NaN, those of out the sentinel) between guards, twice; returns the [M, C] result
    after checking that the pad columns of out are untouched."""
    from anyedit_amd import ops
    M, C = B * H * W, nH * 32
    ldq, ldo = 3 * C + 8, C + 8
    wide = torch.full((M, ldq), float("nan"), dtype=BF)
    wide[:, :3 * C] = qkv
    dq, db, dr = wide.to(DEV), qkv_bias.to(DEV), bias.to(DEV)
    bits = _twice((M, ldo), lambda out: ops.swin_window_attention(dq[:, :3 * C], db, dr, B, H, W, nH, ws, shift, scale, out=out[:, :C]))
    assert bool((bits[:, C:] == torch.tensor(SENT, dtype=torch.int16)).all()), "columns between C and the row stride belong to no token and must stay untouched"
    got = bits[:, :C].contiguous().view(BF)
    assert torch.isfinite(got.float()).all(), "a token's row was not written"
    return got


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nH", [1, 4])
@pytest.mark.parametrize("mapname", list(MAPS))
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("ws", [7, 12])
def test_window_attention_vs_float64(ws, shifted, mapname, nH, B):
    H, W = MAPS[mapname](ws)
    shift = ws // 2 if shifted else 0
    gen = torch.Generator().manual_seed(ws * 1000 + shift * 100 + H * 10 + nH * 2 + B)
    scale = 32 ** -0.5
    C, qkv, qkv_bias, bias = _attn_inputs(ws, nH, B, H, W, gen)
    got = _run_attn(qkv, qkv_bias, bias, B, H, W, nH, ws, shift, scale)
    ref, pav = _attn_float64(qkv, qkv_bias, bias, B, H, W, nH, ws, shift, scale)
    ratio = float(((got.to(F64) - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -8 * pav + 1e-30)).max())
    print(f"swin_window_attention ws={ws} shift={shift} map={H}x{W} heads={nH} B={B}: worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_pad_keys_take_part_in_the_softmax():
    """qkv_bias with b_k = 3 mean(q): the pad keys of a padded window carry most of the softmax weight, so its rows move toward b_v.  float64
    says by how much; a kernel that masked pad keys out would give the float64 answer WITHOUT them, which the attention rule tells apart."""
    ws, nH, B = 7, 4, 1
    H, W = MAPS["pad2x2"](ws)
    scale = 32 ** -0.5
    gen = torch.Generator().manual_seed(77)
    C, qkv, qkv_bias, bias = _attn_inputs(ws, nH, B, H, W, gen, q_offset=torch.randn(nH * 32, generator=gen))
    qkv_bias[C:2 * C] = 3.0 * qkv[:, :C].float().mean(0)
    ref, pav = _attn_float64(qkv, qkv_bias, bias, B, H, W, nH, ws, 0, scale)
    masked_bias = qkv_bias.clone()
    masked_bias[C:2 * C] = -1000.0 * qkv[:, :C].float().mean(0)           # pad keys with logits so low that they carry no weight: "pad keys masked out"
    ref_masked, _ = _attn_float64(qkv, masked_bias, bias, B, H, W, nH, ws, 0, scale)
    got = _run_attn(qkv, qkv_bias, bias, B, H, W, nH, ws, 0, scale).to(F64)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * pav + 1e-30
    bv = qkv_bias[2 * C:].to(BF).to(F64)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sel = ((ys >= ws) | (xs >= ws)).reshape(-1)                            # the rows of the three windows that hold pad keys (window (0, 0) has none)
    d_got, d_ref, d_masked = (float((t[sel] - bv).abs().mean()) for t in (got, ref, ref_masked))
    apart = float(((ref - ref_masked).abs() > 4 * bound)[sel].double().mean())
    print(f"pad keys: mean |out - b_v|: HIP {d_got:.4f}  float64 {d_ref:.4f}  float64 with pad keys masked out {d_masked:.4f}; "
          f"{apart:.2f} of the elements tell the two float64 answers apart by 4 bounds")
    assert d_ref < 0.5 * d_masked and apart > 0.5, "the case does not separate the two behaviours"
    assert float(((got - ref).abs() / bound).max()) <= 1.0
    assert d_got < 0.05 * d_masked, "the rows of the padded windows did not move to b_v"      # float64: the pad keys hold all the weight there, out = b_v up to its rounding


# ------------------------------------------------------------------------------------------------------------ merge + LayerNorm
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", [(2, 2), (3, 5), (7, 4), (50, 38)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [32, 128, 512])
def test_merge_layernorm_vs_float64(C, size, B):
    from anyedit_amd import ops
    H, W = size
    gen = torch.Generator().manual_seed(C * 100 + H * 10 + W + B)
    x = (torch.randn(B * H * W, C, generator=gen) * 1.3 + 0.2).to(BF)
    gamma, beta = 0.25 + 1.5 * torch.rand(4 * C, generator=gen), torch.randn(4 * C, generator=gen) * 0.1
    dx, dg, db = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    M2 = B * ((H + 1) // 2) * ((W + 1) // 2)
    got = _twice((M2, 4 * C), lambda out: ops.swin_merge_layernorm(dx, dg, db, B, H, W, 1e-5, out=out)).view(BF)
    ref = F.layer_norm(R.merge_rows(x.to(F64).view(B, H * W, C), H, W), (4 * C,), gamma.to(F64), beta.to(F64), 1e-5).view(M2, 4 * C)
    ratio = float(((got.to(F64) - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-30)).max())
    print(f"swin_merge_layernorm C={C} map={H}x{W} B={B}: worst |err| / bound {ratio:.3f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ towers
def _weights(geom):
    arrs = {}
    for i in range(len(TINY[geom]["depths"])):
        arrs.update(load_golden(f"swin_tiny_{geom}_w{i}"))
    return R.fixture_state_dict(arrs)


def _tiny(geom):
    from anyedit_amd.groundingdino.swin_transformer import SwinTransformer
    cfg = TINY[geom]
    sd = _weights(geom)
    m = SwinTransformer(out_indices=tuple(range(len(cfg["depths"]))), **cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval().requires_grad_(False), sd


@pytest.mark.parametrize("geom,size", CASES, ids=CASE_IDS)
def test_tiny_tower_vs_reference_golden(geom, size):
    """Every stored output of this image under the tower rule, control = swin_ref(bf16_storage=True) on the same weights: the maps of
    forward_raw (fp32 pixels -> fp32 maps), the input of stage 1 (PatchMerging of stage 0) and, where stored, the masks of forward(NestedTensor)."""
    from anyedit_amd.groundingdino.misc import NestedTensor
    m, sd = _tiny(geom)
    cfg = TINY[geom]
    o = load_golden(f"swin_tiny_{geom}_out_{size[0]}x{size[1]}")
    px = T(o["pixels"])
    ctl = R.swin_forward(sd, px, cfg, bf16_storage=True)
    pd = px.to(DEV)
    outs = m.forward_raw(pd)
    report, ok = [], True
    assert len(outs) == len(cfg["depths"])
    for i, t in enumerate(outs):
        assert t.dtype == torch.float32 and tuple(t.shape) == o[f"out.{i}"].shape and t.is_contiguous()
        ok &= _judge(f"{geom} {size[0]}x{size[1]} out.{i}", t, ctl["outs"][i], T(o[f"out.{i}"]), report)
    st = m.run(pd).stages[1]
    ok &= _judge(f"{geom} {size[0]}x{size[1]} stage1_in", st.x0.view(2, st.H * st.W, st.C), ctl["stage_in"][1], T(o["stage1_in"]), report)
    if "mask_in" in o:
        nested = m(NestedTensor(pd, T(o["mask_in"]).to(DEV)))
        assert sorted(nested) == list(range(len(outs)))
        for i, nt in nested.items():
            assert nt.mask.dtype == torch.bool and torch.equal(nt.mask.cpu(), T(o[f"mask.{i}"])), f"mask {i}"
            assert torch.equal(nt.tensors, outs[i])
    bf = m.forward_raw(pd.to(BF))
    assert all(t.dtype == BF for t in bf)                                  # the maps come in the input's dtype
    print("\n".join(report))
    assert ok, "\n".join(report)


def test_swin_b_widths_vs_restatement():
    """Width 128, heads 4 / 8 / 16 / 32, window 12, two blocks per stage (the real depth of 18 adds time, not coverage), one 200x152 image, seeded
    weights, under the tower rule against swin_ref in fp32."""
    from anyedit_amd.groundingdino.swin_transformer import build_swin_transformer
    cfg = dict(R.GEOMETRIES["swin_B_384_22k"], depths=[2, 2, 2, 2])
    sd = R.seeded_state_dict(cfg, seed=0)
    with torch.device("meta"):
        m = build_swin_transformer("swin_B_384_22k", 384, depths=[2, 2, 2, 2])
    m.load_state_dict(sd, assign=True)
    m = m.to(DEV).eval()
    px = torch.rand(1, 3, 200, 152, generator=torch.Generator().manual_seed(1))
    ref, ctl = R.swin_forward(sd, px, cfg), R.swin_forward(sd, px, cfg, bf16_storage=True)
    outs = m.forward_raw(px.to(DEV))
    assert [tuple(t.shape) for t in outs] == [(1, 128, 50, 38), (1, 256, 25, 19), (1, 512, 13, 10), (1, 1024, 7, 5)]
    report, ok = [], True
    for i, t in enumerate(outs):
        ok &= _judge(f"Swin-B out.{i}", t, ctl["outs"][i], ref["outs"][i], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


def test_swin_l_widths_vs_restatement():
    """The last two stages of Swin-L (widths 768 -> 1536, heads 24 / 48, hidden 3072 / 6144, window 12; the merging normalises 4 * 768 values), two
    blocks each, one 40x56 token map fed as a 160x224 image through a 768-wide patch embedding, seeded weights, under the tower rule."""
    from anyedit_amd.groundingdino.swin_transformer import SwinTransformer
    cfg = dict(embed_dim=768, depths=[2, 2], num_heads=[24, 48], window_size=12)
    sd = R.seeded_state_dict(cfg, seed=3)
    with torch.device("meta"):
        m = SwinTransformer(out_indices=(0, 1), **cfg)
    m.load_state_dict(sd, assign=True)
    m = m.to(DEV).eval()
    assert m.num_features == [768, 1536] and m.layers[1].blocks[0].mlp.fc1.weight.shape == (6144, 1536)
    px = torch.rand(1, 3, 160, 224, generator=torch.Generator().manual_seed(2))
    ref, ctl = R.swin_forward(sd, px, cfg), R.swin_forward(sd, px, cfg, bf16_storage=True)
    outs = m.forward_raw(px.to(DEV))
    assert [tuple(t.shape) for t in outs] == [(1, 768, 40, 56), (1, 1536, 20, 28)]
    report, ok = [], True
    for i, t in enumerate(outs):
        ok &= _judge(f"Swin-L widths out.{i}", t, ctl["outs"][i], ref["outs"][i], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


def test_dilated_tower_vs_restatement():
    """dilation=True: the last merging is dropped and the last stage runs at the size and width of the one before it (its input is a copy of that
    stage's output).  Tiny widths with head dim 32 everywhere, seeded weights, under the tower rule against swin_ref (which reads the downsampling
    from the state dict)."""
    from anyedit_amd.groundingdino.swin_transformer import SwinTransformer
    cfg = dict(embed_dim=32, depths=[2, 2, 2], num_heads=[1, 2, 2], window_size=7)
    sd = R.seeded_state_dict(cfg, seed=5, dilation=True)
    m = SwinTransformer(out_indices=(0, 1, 2), dilation=True, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    assert m.num_features == [32, 64, 64] and "layers.1.downsample.reduction.weight" not in sd and "layers.0.downsample.reduction.weight" in sd
    px = torch.rand(2, 3, 50, 38, generator=torch.Generator().manual_seed(4))
    ref, ctl = R.swin_forward(sd, px, cfg), R.swin_forward(sd, px, cfg, bf16_storage=True)
    outs = m.forward_raw(px.to(DEV))
    assert [tuple(t.shape) for t in outs] == [(2, 32, 13, 10), (2, 64, 7, 5), (2, 64, 7, 5)]
    report, ok = [], True
    for i, t in enumerate(outs):
        ok &= _judge(f"dilated out.{i}", t, ctl["outs"][i], ref["outs"][i], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ behaviour
def test_the_bias_follows_its_table():
    """An in-place change of relative_position_bias_table changes the output, and the new output is the restatement's with the new table."""
    m, sd = _tiny("a")
    cfg = TINY["a"]
    px = T(load_golden("swin_tiny_a_out_50x38")["pixels"])
    before = [t.clone() for t in m.forward_raw(px.to(DEV))]
    key = "layers.0.blocks.1.attn.relative_position_bias_table"
    with torch.no_grad():
        m.layers[0].blocks[1].attn.relative_position_bias_table.neg_()
    sd2 = dict(sd)
    sd2[key] = -sd[key]
    after = m.forward_raw(px.to(DEV))
    assert all(not torch.equal(a, b) for a, b in zip(after, before)), "the packed bias did not follow the parameter"
    ref, ctl = R.swin_forward(sd2, px, cfg), R.swin_forward(sd2, px, cfg, bf16_storage=True)
    report = []
    ok = all([_judge(f"negated table out.{i}", t, ctl["outs"][i], ref["outs"][i], report) for i, t in enumerate(after)])
    print("\n".join(report))
    assert ok, "\n".join(report)


@pytest.mark.parametrize("geom", ["a", "b"])
def test_maps_do_not_depend_on_the_batch(geom):
    m, _ = _tiny(geom)
    size = SIZES[geom][0]
    px = T(load_golden(f"swin_tiny_{geom}_out_{size[0]}x{size[1]}")["pixels"]).to(DEV)
    both = [t.clone() for t in m.forward_raw(px)]
    for b in range(2):
        alone = m.forward_raw(px[b:b + 1].contiguous())
        for i, t in enumerate(alone):
            assert torch.equal(both[i][b:b + 1], t), f"image {b}, map {i}: running it with a neighbour changed it"


def test_forward_is_capturable_and_allocates_nothing_after_the_first_call():
    m, _ = _tiny("a")
    px = T(load_golden("swin_tiny_a_out_50x38")["pixels"])
    static_px = px.to(DEV)
    first = [t.clone() for t in m.forward_raw(static_px)]
    m.forward_raw(static_px)
    torch.cuda.synchronize()
    before, mem = torch.cuda.memory_stats(DEV)["allocation.all.allocated"], torch.cuda.memory_allocated(DEV)
    for _ in range(5):
        last = m.forward_raw(static_px)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before, "a forward after the first allocated"
    assert torch.cuda.memory_allocated(DEV) == mem
    assert all(torch.equal(a, b) for a, b in zip(last, first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward_raw(static_px)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, no side branches: the tower only ever uses the current stream
        outs = m.forward_raw(static_px)
    new_px = px.flip(0).contiguous()
    static_px.copy_(new_px.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    eager = [t.clone() for t in m.forward_raw(new_px.to(DEV))]
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager)), "graph replay differs from the eager forward of the same pixels"
    assert not torch.equal(replayed[0], first[0])


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from anyedit_amd import ops
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=DEV)
    qkv, qb, rpb = z(49, 96), z(96, dt=torch.float32), z(1, 49, 49, dt=torch.float32)
    ok = lambda **kw: ops.swin_window_attention(**dict(dict(qkv=qkv, qkv_bias=qb, bias=rpb, B=1, H=7, W=7, heads=1, window=7, shift=0, scale=0.17), **kw))
    assert ok().shape == (49, 32)
    with pytest.raises(ValueError, match="head_dim 64/1 must be 32"):
        ok(qkv=z(49, 192), qkv_bias=z(192, dt=torch.float32))
    with pytest.raises(ValueError, match="window size 17"):
        ok(window=17)
    with pytest.raises(ValueError, match="shift 7"):
        ok(shift=7)
    with pytest.raises(ValueError, match="49 rows are not"):
        ok(H=8)
    with pytest.raises(ValueError, match=r"bias must be a contiguous \[1, 49, 49\]"):
        ok(bias=z(1, 49, 50, dt=torch.float32)[:, :, :49])
    with pytest.raises(TypeError, match="qkv"):
        ok(qkv=z(49, 96, dt=torch.float32))
    with pytest.raises(ValueError, match="GPU tensor"):
        ok(qkv=torch.zeros(49, 96, dtype=BF))
    with pytest.raises(ValueError, match="out must be"):
        ok(out=z(49, 64))
    x, g = z(12, 32), z(128, dt=torch.float32)
    assert ops.swin_merge_layernorm(x, g, g, 1, 3, 4).shape == (4, 128)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.swin_merge_layernorm(z(12, 36), z(144, dt=torch.float32), z(144, dt=torch.float32), 1, 3, 4)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.swin_merge_layernorm(z(12, 1032), z(4128, dt=torch.float32), z(4128, dt=torch.float32), 1, 3, 4)
    with pytest.raises(ValueError, match="4C = 128"):
        ops.swin_merge_layernorm(x, z(64, dt=torch.float32), g, 1, 3, 4)
    with pytest.raises(ValueError, match=r"\[1\*3\*5, C\]"):
        ops.swin_merge_layernorm(x, g, g, 1, 3, 5)
    torch.cuda.synchronize()
