"""GPU tests of GroundingDINO's feature enhancer: its two attention kernels against float64 between sentinel guards (launched twice,
bit-identical), both tiny towers against the reference's golden and a production-width tower against the restatement (under the project's
1.5 x control rule), the order of the sub-blocks, batch independence, graph capture and the refusals.  Every case runs once.

Two comparison rules.  Attention rule (tests/test_hip_swin.py, tests/test_hip_clip_text.py): every element within 2^-8 |ref| + 2^-8 (P @ |V|) +
1e-30 of the float64 result computed from the same bf16 inputs — one bf16 rounding of the output plus one of every probability.  Tower rule:
rel-L2 error of the HIP tower <= 1.5 x the error of the control (the fp32 restatement rounding to bf16 wherever the HIP path stores bf16), both
against the same fp32 reference."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, rel_l2, T  # noqa: E402
import gdino_enc_ref as R  # noqa: E402
from gdino_enc_ref import GEOMS, module, run_restatement, stored, weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
SENT = 0x7FA5          # a NaN bit pattern no kernel writes
GUARD = 4096
D_BI = 256


def _guarded(shape):
    """A bf16 buffer of `shape` between two sentinel-filled guard bands, itself pre-filled with the sentinel."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, dtype=BF, device=DEV)
    buf.view(torch.int16).fill_(SENT)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    iv = buf.view(torch.int16)
    return bool((iv[:GUARD] == SENT).all()) and bool((iv[-GUARD:] == SENT).all())


def _worst(got, ref, pav):
    return float(((got.to(F64) - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -8 * pav + 1e-30)).max())


# ------------------------------------------------------------------------------------------------------------------ bi-attention
def _split_points():
    """(smallest Nv the text direction takes in two partials, an Nv of three partials with a ragged last one) from the kernel's own plan."""
    from anyedit_amd import ops
    parts = lambda nv: -(-nv // ops.bi_attention_split_rows(nv))
    two = next(nv for nv in range(1, 1 << 16) if parts(nv) == 2)
    rows = ops.bi_attention_split_rows(two)
    three = 2 * rows + 37
    assert parts(two - 1) == 1 and parts(three) == 3 and ops.bi_attention_split_rows(three) == rows and three % rows not in (0, rows)
    return two, three


def _bi_inputs(B, Nv, Nt, heads, gen):
    C = heads * D_BI
    mk = lambda n: torch.randn(B, n, C, generator=gen).to(BF)
    return mk(Nv), mk(Nt), mk(Nv), mk(Nt)


def _run_bi(q, k, vv, vl, heads, scale, mask_v=None, mask_l=None):
    """ops.bi_attention on strided rows (the pad columns of the inputs hold NaN, those of the outputs the sentinel) between guards, twice."""
    from anyedit_amd import ops
    B, Nv, C = q.shape
    Nt = k.shape[1]
    ld = C + 8

    def wide(t):
        w = torch.full((t.shape[0], t.shape[1], ld), float("nan"), dtype=BF)
        w[..., :C] = t
        return w.to(DEV)[..., :C]

    dq, dk, dvv, dvl = wide(q), wide(k), wide(vv), wide(vl)
    mv = None if mask_v is None else mask_v.to(DEV)
    ml = None if mask_l is None else mask_l.to(DEV)
    runs = []
    for _ in range(2):
        bv, ov = _guarded((B, Nv, ld))
        bl, ol = _guarded((B, Nt, ld))
        r = ops.bi_attention(dq, dk, dvv, dvl, heads, scale, mv, ml, out_v=ov[..., :C], out_l=ol[..., :C])
        torch.cuda.synchronize()
        assert r[0].data_ptr() == ov.data_ptr() and r[1].data_ptr() == ol.data_ptr()
        assert _guards_intact(bv) and _guards_intact(bl), "wrote outside its outputs"
        runs.append((ov.clone().view(torch.int16).cpu(), ol.clone().view(torch.int16).cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
    outs = []
    for bits in runs[0]:
        assert bool((bits[..., C:] == torch.tensor(SENT, dtype=torch.int16)).all()), "columns between heads*D and the row stride must stay untouched"
        got = bits[..., :C].contiguous().view(BF)
        assert torch.isfinite(got.float()).all(), "a row was not written, or is not finite"
        outs.append(got)
    return outs


def _masks(kind, B, Nv, Nt, gen):
    """none | both (random padding, at least one live token each) | tail (the trailing image tile of 64, or all but one token, is padding)."""
    if kind == "none":
        return None, None
    mv = torch.zeros(B, Nv, dtype=torch.bool)
    ml = torch.zeros(B, Nt, dtype=torch.bool)
    if kind == "both":
        mv = torch.rand(B, Nv, generator=gen) < 0.3
        ml = torch.rand(B, Nt, generator=gen) < 0.3
        mv[:, int(torch.randint(Nv, (1,), generator=gen))] = False
        ml[:, int(torch.randint(Nt, (1,), generator=gen))] = False
    else:
        keep = max(1, (Nv - 1) // 64 * 64 if Nv > 64 else 1)         # everything from the start of the last 64-token tile on is padding
        mv[:, keep:] = True
        ml[:, Nt // 2 + 1:] = True
    return mv, ml


def _bi_case(B, Nv, Nt, heads, kind, seed, k_offset=0.0):
    gen = torch.Generator().manual_seed(seed)
    scale = D_BI ** -0.5
    q, k, vv, vl = _bi_inputs(B, Nv, Nt, heads, gen)
    if k_offset:
        k = (k.float() + k_offset).to(BF)
    mv, ml = _masks(kind, B, Nv, Nt, gen)
    got_v, got_l = _run_bi(q, k, vv, vl, heads, scale, mv, ml)
    ref_v, ref_l, pav_v, pav_l = R.bi_attention_float64(q, k, vv, vl, heads, scale, mv, ml)
    rv, rl = _worst(got_v, ref_v, pav_v), _worst(got_l, ref_l, pav_l)
    print(f"bi_attention B={B} Nv={Nv} Nt={Nt} heads={heads} masks={kind} k_offset={k_offset}: worst |err| / bound  out_v {rv:.3f}  out_l {rl:.3f}")
    return rv, rl


BASE = dict(B=2, Nv=65, Nt=33, heads=1, kind="both")


@pytest.mark.parametrize("Nv", [1, 63, 64, 65, "two", "three"])
def test_bi_attention_vs_float64_over_image_tokens(Nv):
    if isinstance(Nv, str):
        Nv = _split_points()[0 if Nv == "two" else 1]
    rv, rl = _bi_case(**dict(BASE, Nv=Nv), seed=1000 + Nv)
    assert rv <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("Nt", [1, 7, 33, 256])
def test_bi_attention_vs_float64_over_text_tokens(Nt):
    rv, rl = _bi_case(**dict(BASE, Nt=Nt), seed=2000 + Nt)
    assert rv <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("heads,B", [(1, 1), (4, 1), (4, 2)])
def test_bi_attention_vs_float64_over_heads_and_samples(heads, B):
    rv, rl = _bi_case(**dict(BASE, heads=heads, B=B), seed=3000 + 10 * heads + B)
    assert rv <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("kind", ["none", "both", "tail"])
def test_bi_attention_vs_float64_over_masks(kind):
    """On three partials with a ragged last one: `tail` leaves the last partial (and the last 64-token tile) without a single live key."""
    rv, rl = _bi_case(**dict(BASE, Nv=_split_points()[1], Nt=40, heads=2, kind=kind), seed=4000 + len(kind))
    assert rv <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("span", [80.0, 150.0])
def test_bi_attention_subtracts_a_maximum_on_both_axes(span):
    """A column offset of span / 3 on k moves the logits of image token i by (span / 3) x N(0, 1): over a few hundred image tokens they reach
    about +-span.  The image direction sees the offset as one constant per row (it tests that a large row is shifted down before exp), the text
    direction sees its whole spread along the softmax axis.  span = 80 is the magnitude the kernel was specified against; exp(80) = 5.5e34 is
    still finite in fp32, so only span = 150 (exp overflows from 88.7 on, and exp(-104) is already zero) makes a missing subtraction on either
    axis certain to give inf / NaN or 0 / 0 rather than likely."""
    Nv = _split_points()[1]
    rv, rl = _bi_case(**dict(BASE, Nv=Nv, Nt=40, heads=2, kind="none"), seed=5000, k_offset=span / 3.0)
    assert rv <= 1.0 and rl <= 1.0


def test_bi_attention_mask_sense():
    """True = padded = removed as a key.  A masked text key and a masked image key carry logits about 20 above every other: float64 with and
    without the masks differ by far more than the bound, and the kernel must give the masked answer."""
    B, Nv, Nt, heads = 2, 70, 20, 1
    gen = torch.Generator().manual_seed(6000)
    scale = D_BI ** -0.5
    q, k, vv, vl = _bi_inputs(B, Nv, Nt, heads, gen)
    u = torch.full((heads * D_BI,), 0.5)
    q, k = q.float() + u, k.float() + u                 # scale u.u = 4 on every logit
    jstar, istar = 5, 66
    k[:, jstar] += 5.0 * u                              # + scale 5 q_i.u ~ 20 for every image token
    q[:, istar] += 5.0 * u                              # + 20 for every text token
    q, k = q.to(BF), k.to(BF)
    mv = torch.zeros(B, Nv, dtype=torch.bool)
    ml = torch.zeros(B, Nt, dtype=torch.bool)
    mv[:, istar] = True
    ml[:, jstar] = True
    ref_v, ref_l, pav_v, pav_l = R.bi_attention_float64(q, k, vv, vl, heads, scale, mv, ml)
    un_v, un_l, _, _ = R.bi_attention_float64(q, k, vv, vl, heads, scale, None, None)
    assert _worst(un_v, ref_v, pav_v) > 10.0 and _worst(un_l, ref_l, pav_l) > 10.0, "the masked keys must matter"
    inv_v, inv_l, _, _ = R.bi_attention_float64(q, k, vv, vl, heads, scale, ~mv, ~ml)
    assert _worst(inv_v, ref_v, pav_v) > 10.0 and _worst(inv_l, ref_l, pav_l) > 10.0
    got_v, got_l = _run_bi(q, k, vv, vl, heads, scale, mv, ml)
    rv, rl = _worst(got_v, ref_v, pav_v), _worst(got_l, ref_l, pav_l)
    print(f"bi_attention mask sense: worst |err| / bound  out_v {rv:.3f}  out_l {rl:.3f}")
    assert rv <= 1.0 and rl <= 1.0


def test_bi_attention_warm_call_allocates_nothing():
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(6500)
    q, k, vv, vl = (t.to(DEV) for t in _bi_inputs(1, 300, 16, 1, gen))
    ov, ol = torch.empty_like(q), torch.empty_like(k)
    ops.bi_attention(q, k, vv, vl, 1, 0.0625, out_v=ov, out_l=ol)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    for _ in range(3):
        ops.bi_attention(q, k, vv, vl, 1, 0.0625, out_v=ov, out_l=ol)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before, "a warmed-up bi_attention allocated"


# ------------------------------------------------------------------------------------------------------------------ masked short attention
def _allowed(kind, BH, N, gen):
    if kind == "ones":
        return torch.ones(BH, N, N, dtype=torch.bool)
    a = torch.eye(N, dtype=torch.bool).repeat(BH, 1, 1)
    if kind == "block":                                   # block-diagonal, other blocks in every (batch, head) slice
        for s in range(BH):
            cuts = sorted(set([0, N] + torch.randint(0, N + 1, (3,), generator=gen).tolist()))
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                a[s, lo:hi, lo:hi] = True
    return a


def _masked_case(N, D, H, B, kind, seed):
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(seed)
    C = H * D
    ldq = 2 * C + 8
    qk = torch.full((B * N, ldq), float("nan"), dtype=BF)                    # the module's packed q | k rows, with pad columns
    qk[:, :2 * C] = torch.randn(B * N, 2 * C, generator=gen).to(BF)
    v = torch.randn(B * N, C, generator=gen).to(BF)
    allowed = _allowed(kind, B * H, N, gen)
    dqk, dv, dm = qk.to(DEV), v.to(DEV), allowed.to(DEV)
    scale = D ** -0.5
    bits = []
    for _ in range(2):
        buf, out = _guarded((B, N, C))
        ops.attention_masked_short(dqk, dqk[:, C:], dv, dm, B, H, N, D, scale, (N * ldq, D, ldq), (N * ldq, D, ldq), (N * C, D, C), out=out)
        torch.cuda.synchronize()
        assert _guards_intact(buf), "wrote outside its output"
        bits.append(out.clone().view(torch.int16).cpu())
    assert torch.equal(bits[0], bits[1]), "two launches differ"
    got = bits[0].view(BF)
    assert torch.isfinite(got.float()).all(), "a row was not written"
    q3, k3, v3 = qk[:, :C].reshape(B, N, C), qk[:, C:2 * C].reshape(B, N, C), v.view(B, N, C)
    ref, pav = R.masked_attention_float64(q3, k3, v3, allowed, H, scale)
    ratio = _worst(got, ref, pav)
    print(f"attention_masked_short N={N} D={D} H={H} B={B} mask={kind}: worst |err| / bound {ratio:.3f}")
    if kind == "block" and B * H > 1 and N >= 17:            # the masks of the (batch, head) slices are not interchangeable
        other, _ = R.masked_attention_float64(q3, k3, v3, allowed.roll(1, 0), H, scale)
        assert _worst(got, other, pav) > 1.0, "every slice must read its own mask"
    return ratio


@pytest.mark.parametrize("kind", ["diag", "block", "ones"])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("N", [1, 17, 128, 129, 256])
def test_attention_masked_short_vs_float64(N, D, kind):
    assert _masked_case(N, D, 4, 2, kind, 7000 + 10 * N + D + len(kind)) <= 1.0


@pytest.mark.parametrize("H,B", [(1, 1), (1, 2), (4, 1)])
@pytest.mark.parametrize("D", [32, 64])
def test_attention_masked_short_vs_float64_over_heads_and_samples(D, H, B):
    assert _masked_case(129, D, H, B, "block", 8000 + D + 10 * H + B) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ towers
def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


@functools.lru_cache(maxsize=None)
def _tiny(geom):
    from anyedit_amd.checkpoints import load_groundingdino_encoder
    m = module(geom)
    load_groundingdino_encoder(m, weights(geom))
    return m.to(DEV).eval()


def _tiny_inputs(geom, sample=None):
    o = stored(geom)
    sl = (lambda t: t) if sample is None else (lambda t: t[sample:sample + 1])
    d = lambda name: sl(T(o[name])).to(DEV)
    return dict(src=d("src"), pos=d("pos"), spatial_shapes=T(o["spatial_shapes"]).to(DEV), level_start_index=T(o["level_start_index"]).to(DEV),
                valid_ratios=d("valid_ratios"), key_padding_mask=d("key_padding_mask"), memory_text=d("memory_text"),
                text_attention_mask=d("text_attention_mask"), pos_text=d("pos_text"), text_self_attention_masks=d("text_self_attention_masks"))


@functools.lru_cache(maxsize=None)
def _tiny_control(geom):
    taps = {}
    out = run_restatement(geom, store=R.round_bf16, tap=lambda i, n, x, t: taps.__setitem__((i, n), (x, t)))
    return out, taps


@pytest.mark.parametrize("geom", list(GEOMS))
def test_tiny_tower_matches_the_reference_golden(geom):
    o, m = stored(geom), _tiny(geom)
    with torch.no_grad():
        out, text = m(**_tiny_inputs(geom))
    assert out.dtype == torch.float32 and text.dtype == torch.float32 and out.shape == o["out"].shape and text.shape == o["out_text"].shape
    (c_out, c_text), _ = _tiny_control(geom)
    report = []
    ok = [_judge(f"{geom} image stream", out, c_out, T(o["out"]), report), _judge(f"{geom} text stream", text, c_text, T(o["out_text"]), report)]
    print("\n".join(report))
    assert all(ok), report


def test_sub_blocks_run_in_the_reference_s_order():
    """Geometry a, layer 0: the stream each sub-block leaves against the reference's forward-hook captures."""
    o, m = stored("a"), _tiny("a")
    seen = {}
    m.tap = lambda i, n, x, t: seen.__setitem__((i, n), (x.clone(), t.clone()))
    try:
        with torch.no_grad():
            m(**_tiny_inputs("a"))
    finally:
        m.tap = None
    assert list(seen)[:3] == [(0, "fusion"), (0, "text"), (0, "deform")]
    _, ctl = _tiny_control("a")
    report, ok = [], []
    for name, streams in (("fusion", "vl"), ("text", "l"), ("deform", "v")):
        for s in streams:
            idx = 0 if s == "v" else 1
            ref = T(o[f"tap.0.{name}.{s}"])
            ok.append(_judge(f"layer 0 after {name}, stream {s}", seen[(0, name)][idx].view(ref.shape), ctl[(0, name)][idx], ref, report))
    print("\n".join(report))
    assert all(ok), report


@functools.lru_cache(maxsize=None)
def _production():
    """d_model 256, nhead 8, dim_feedforward 2048, 2 layers, four levels, 40 text tokens, the position_ids path; seeded weights."""
    from anyedit_amd.groundingdino.transformer import build_feature_enhancer
    levels = [(20, 15), (10, 8), (5, 4), (3, 2)]
    gen = torch.Generator().manual_seed(9000)
    m = build_feature_enhancer(d_model=256, nhead=8, dim_feedforward=2048, num_layers=2, num_feature_levels=4, enc_n_points=4)
    sd = R.draw_weights(m.state_dict(), gen)
    m.load_state_dict(sd, strict=True)
    B, C, Nt = 2, 256, 40
    Nv = sum(h * w for h, w in levels)
    starts = [0]
    for h, w in levels[:-1]:
        starts.append(starts[-1] + h * w)
    kpm = torch.zeros(B, Nv, dtype=torch.bool)
    ratios = torch.ones(B, 4, 2)
    for l, (h, w) in enumerate(levels):                       # sample 1: the right quarter of every level is padding
        vw = max(1, w - max(1, w // 4))
        mk = torch.zeros(h, w, dtype=torch.bool)
        mk[:, vw:] = True
        kpm[1, starts[l]:starts[l] + h * w] = mk.reshape(-1)
        ratios[1, l, 0] = vw / w
    tmask = torch.zeros(B, Nt, dtype=torch.bool)
    tmask[1, 29:] = True
    tsam = torch.eye(Nt, dtype=torch.bool).repeat(B, 1, 1)
    ids = torch.zeros(B, Nt, dtype=torch.long)
    for b, cuts in enumerate(([0, 1, 9, 20, 39, 40], [0, 1, 5, 17, 28, 29])):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            tsam[b, lo:hi, lo:hi] = True
            ids[b, lo:hi] = torch.arange(hi - lo)
    inp = dict(src=torch.randn(B, Nv, C, generator=gen), pos=0.5 * torch.randn(B, Nv, C, generator=gen), spatial_shapes=torch.tensor(levels),
               level_start_index=torch.tensor(starts), valid_ratios=ratios, key_padding_mask=kpm, memory_text=torch.randn(B, Nt, C, generator=gen),
               text_attention_mask=tmask, text_self_attention_masks=tsam, position_ids=ids)
    cfg = dict(num_layers=2, nhead=8, enc_n_points=4)
    run = lambda store: R.encoder_forward(sd, cfg, inp["src"], inp["pos"], levels, ratios, kpm, inp["memory_text"], tmask, text_self_attention_masks=tsam,
                                          position_ids=ids, store=store)
    return m.to(DEV).eval(), {k: v.to(DEV) for k, v in inp.items()}, run(None), run(R.round_bf16)


def test_production_width_tower_vs_restatement():
    m, inp, ref, ctl = _production()
    with torch.no_grad():
        out, text = m(**inp)
    report = []
    ok = [_judge("production image stream", out, ctl[0], ref[0], report), _judge("production text stream", text, ctl[1], ref[1], report)]
    print("\n".join(report))
    assert torch.isfinite(out).all() and torch.isfinite(text).all()
    assert all(ok), report


def test_a_sample_does_not_depend_on_its_neighbour():
    """Geometry a has one text head, so the reference's mask indexing (sample (b nhead + h) mod bs) reads every sample's own mask."""
    m = _tiny("a")
    with torch.no_grad():
        both = [t.clone() for t in m(**_tiny_inputs("a"))]
        alone = [t.clone() for t in m(**_tiny_inputs("a", sample=0))]
    for name, a, b in zip(("image", "text"), alone, both):
        assert torch.equal(a[0], b[0]), f"{name} stream of sample 0 changed with a neighbour in the batch"


def test_two_level_sets_of_equal_token_count_through_one_module():
    """The reference builds a fresh GPU spatial_shapes per image (transformer.py:244-246); freed after the call, the next one commonly lands at
    the same address with the same version.  Geometry a's 89 tokens as (9,7) (5,4) (3,2), then as (7,9) (4,5) (2,3) through the SAME module: the
    second call must run on the second set's sizes (the restatement of that set judges it under the tower rule) and not repeat the first."""
    o, m = stored("a"), _tiny("a")
    sets = [GEOMS["a"]["levels"], [(w, h) for h, w in GEOMS["a"]["levels"]]]
    assert sets[0] != sets[1] and sum(h * w for h, w in sets[0]) == sum(h * w for h, w in sets[1])
    outs, ptrs = [], []
    for levels in sets + [sets[0]]:
        inp = _tiny_inputs("a")
        del inp["spatial_shapes"]
        shapes = torch.as_tensor(levels, dtype=torch.long, device=DEV)          # a fresh tensor per call, as the reference makes it
        ptrs.append(shapes.data_ptr())
        with torch.no_grad():
            outs.append([t.clone() for t in m(spatial_shapes=shapes, **inp)])
        del shapes
    print(f"spatial_shapes addresses of the three calls: {ptrs}")
    assert not torch.equal(outs[0][0], outs[1][0]), "the second level set gave the first one's result"
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1]), "back on the first set, the first result must return"
    ref = run_restatement("a", levels=sets[1])
    ctl = run_restatement("a", store=R.round_bf16, levels=sets[1])
    assert rel_l2(ref[0], T(o["out"])) > 1e-2, "the two level sets must differ by far more than rounding"
    report = []
    ok = [_judge("swapped levels, image stream", outs[1][0], ctl[0], ref[0], report), _judge("swapped levels, text stream", outs[1][1], ctl[1], ref[1], report)]
    print("\n".join(report))
    assert all(ok), report


def test_forward_captures_and_replays_without_allocating():
    """With the spatial_shapes tensor object of the eager forward before it (whose sizes are reused: a read-back is impossible while
    capturing) the forward captures; a replay allocates nothing and is bit-identical to the eager forward of the same inputs."""
    m = _tiny("a")
    inp = _tiny_inputs("a")
    static = {k: v.clone() for k, v in inp.items()}
    with torch.no_grad():
        first = [t.clone() for t in m(**static)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm the side stream's workspace and caches
            m(**static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        m(**static)                                        # the eager forward whose spatial_shapes object the capture may reuse
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                      # one stream, no side branches: the tower only ever uses the current stream
            outs = m(**static)
        new_src = inp["src"].flip(1).contiguous()
        static["src"].copy_(new_src)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before, "a replay allocated"
        replayed = [t.clone() for t in outs]
        eager = [t.clone() for t in m(**dict(inp, src=new_src))]
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager)), "graph replay differs from the eager forward of the same inputs"
    assert not torch.equal(replayed[0], first[0])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_limit():
    from anyedit_amd import ops
    from anyedit_amd._lib import AnyEditHipError, lib
    z = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="head_dim .* must be 256"):
        ops.bi_attention(z(1, 8, 128), z(1, 4, 128), z(1, 8, 128), z(1, 4, 128), 1, 1.0)
    with pytest.raises(ValueError, match="257 text tokens.*256"):
        ops.bi_attention(z(1, 8, 256), z(1, 257, 256), z(1, 8, 256), z(1, 257, 256), 1, 1.0)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    a, b = z(1, 8, 256), z(1, 4, 256)
    args = lambda Nt, D: (a.data_ptr(), 256, b.data_ptr(), 256, a.data_ptr(), 256, b.data_ptr(), 256, None, None, a.data_ptr(), 256, b.data_ptr(), 256,
                          1, 1, 8, Nt, D, 1.0, ws.data_ptr(), ws.numel(), None)
    assert lib.ae_biattn_bf16(*args(4, 128)) != 0 and b"must be 256" in lib.ae_last_error()
    assert lib.ae_biattn_bf16(*args(257, 256)) != 0 and b"outside [1, 256]" in lib.ae_last_error()
    with pytest.raises(ValueError, match="257.*between 1 and 256"):
        ops.attention_masked_short(z(257, 64), z(257, 64), z(257, 64), torch.ones(1, 257, 257, dtype=torch.uint8, device=DEV), 1, 1, 257, 64, 0.125,
                                   (257 * 64, 64, 64), (257 * 64, 64, 64), (257 * 64, 64, 64))
    with pytest.raises(ValueError, match="head_dim 128"):
        ops.attention_masked_short(z(8, 128), z(8, 128), z(8, 128), torch.ones(1, 8, 8, dtype=torch.uint8, device=DEV), 1, 1, 8, 128, 0.1,
                                   (8 * 128, 128, 128), (8 * 128, 128, 128), (8 * 128, 128, 128))
    x = z(8, 64)
    assert lib.ae_attn_masked_short_bf16(x.data_ptr(), x.data_ptr(), x.data_ptr(), ws.data_ptr(), x.data_ptr(), 1, 1, 257, 64, 0, 64, 64, 0, 64, 64, 0, 64, 64,
                                         0, 64, 64, 0.125, None) != 0
    assert b"outside [1, 256]" in lib.ae_last_error()
    from anyedit_amd.groundingdino.utils import _get_activation_fn
    with pytest.raises(NotImplementedError, match="gelu"):
        _get_activation_fn("gelu")
    m = _tiny("a")
    inp = _tiny_inputs("a")
    try:
        m.train()
        with torch.no_grad(), pytest.raises(RuntimeError, match="train\\(\\) mode with a non-zero dropout"):
            m(**inp)
    finally:
        m.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        m(**inp)                                                   # gradients enabled on parameters
    assert AnyEditHipError is not None
