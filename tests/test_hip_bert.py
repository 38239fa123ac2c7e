"""GPU tests of GroundingDINO's text side: the span attention kernel against float64 at every length where it takes another path, the span /
position-id kernel against the reference's stored masks and the restated rule, the fused embedding LayerNorm against float64, the tiny towers
against the transformers goldens and the full-size tower against the restatement (both under the project's 1.5 x control rule), graph
capture without allocations, and the text_dict going straight into `Transformer.forward`.  Every case runs once."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2, T  # noqa: E402
import bert_ref as R  # noqa: E402
import norm_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F64 = torch.bfloat16, torch.float64
SPECIAL = [1, 2, 3, 4]
GUARD, SENTINEL = 64, -777.0


# ------------------------------------------------------------------------------------------------------------ span attention
def _layout(kind, B, N, gen):
    """int64 [B, N, 2] spans with 0 <= lo < hi <= N."""
    ar = torch.arange(N)
    if kind == "full":
        s = torch.stack([torch.zeros(N, dtype=torch.long), torch.full((N,), N)], -1).expand(B, N, 2)
    elif kind == "single":
        s = torch.stack([ar, ar + 1], -1).expand(B, N, 2)
    elif kind == "partition":          # seeded segments that straddle 16-key and 64-key boundaries and differ per sample
        lens = torch.tensor([1, 2, 3, 7, 13, 16, 17, 30, 33, 64, 70])
        s = torch.zeros(B, N, 2, dtype=torch.long)
        for b in range(B):
            n = 0
            while n < N:
                ln = min(int(lens[torch.randint(0, len(lens), (1,), generator=gen)]), N - n)
                s[b, n:n + ln, 0], s[b, n:n + ln, 1] = n, n + ln
                n += ln
    else:                              # "midtile": the first 64-query block attends keys of the second 64-key tile only; the rest attend everything
        assert N >= 128
        s = torch.stack([torch.zeros(N, dtype=torch.long), torch.full((N,), N)], -1).expand(B, N, 2).clone()
        s[:, :64, 0], s[:, :64, 1] = 70, 100
    return s.contiguous()


def _span_reference(qkv, spans, B, H, N):
    C = H * 64
    sp = lambda t: t.to(F64).view(B, N, H, 64).transpose(1, 2)
    q, k, v = (sp(t) for t in qkv.view(B, N, 3 * C).split(C, -1))
    logits = (q @ k.transpose(-1, -2)) * 64 ** -0.5
    logits = logits.masked_fill(~R.spans_to_mask(spans)[:, None], float("-inf"))
    P = logits.softmax(-1)
    ref = (P @ v).transpose(1, 2).reshape(B, N, C)
    bnd = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * (P @ v.abs()).transpose(1, 2).reshape(B, N, C) + 1e-30
    return ref, bnd, v.transpose(1, 2).reshape(B, N, C)


def _span_launch(qkv_d, spans_d, B, H, N, dense_d=None):
    """attention_span_short between sentinel guards; with `dense_d` (uint8 [B*H, N, N]) attention_masked_short on the same q, k, v instead."""
    from anyedit_amd import ops
    C = H * 64
    buf = torch.full((B * N * C + 2 * GUARD,), SENTINEL, dtype=BF, device=DEV)
    out = buf[GUARD:GUARD + B * N * C].view(B, N, C)
    st = (N * 3 * C, 64, 3 * C)
    if dense_d is None:
        ops.attention_span_short(qkv_d, qkv_d[:, C:], qkv_d[:, 2 * C:], spans_d, B, H, N, 64, 64 ** -0.5, st, st, st, out=out)
    else:
        ops.attention_masked_short(qkv_d, qkv_d[:, C:], qkv_d[:, 2 * C:], dense_d, B, H, N, 64, 64 ** -0.5, st, st, st, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "a store outside the output"
    return out.clone()


_SPAN_CASES = [(N, B, H, kind) for N in (1, 2, 15, 16, 17, 63, 64, 65, 128, 255, 256) for (B, H) in ((1, 1), (2, 12))
               for kind in ("full", "single", "partition", "midtile") if kind != "midtile" or N >= 128]


@pytest.mark.parametrize("N,B,H,kind", _SPAN_CASES)
def test_span_attention_vs_float64(N, B, H, kind):
    """Every element under the project's attention bound |err| <= 2^-8 |ref| + 2^-8 (P @ |V|) (one bf16 rounding of the result and one of the
    probabilities), between sentinel guards; a second launch is bit-identical; a query with one key returns that key's v row exactly; k and
    v rows outside every span of their sample may hold anything."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * H + len(kind))
    C = H * 64
    qkv = torch.randn(B * N, 3 * C, generator=gen).to(BF)
    spans = _layout(kind, B, N, gen)
    ref, bnd, v = _span_reference(qkv, spans, B, H, N)
    qkv_d, spans_d = qkv.to(DEV), spans.to(torch.int32).to(DEV)
    got = _span_launch(qkv_d, spans_d, B, H, N)
    ratio = float(((got.cpu().to(F64) - ref).abs() / bnd).max())
    print(f"span attention N={N} B={B} H={H} {kind}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(_span_launch(qkv_d, spans_d, B, H, N), got), "a second launch differs"
    one = (spans[..., 1] - spans[..., 0]) == 1
    if bool(one.any()):
        assert torch.equal(got.cpu().to(F64)[one], v[one]), "a query with one key must return that key's v row exactly"
    cut = max(1, (3 * N) // 4)
    if cut < N:                        # spans clipped below `cut`: the rows from `cut` on are outside every span
        lo = spans[..., 0].clamp(max=cut - 1)
        clipped = torch.stack([lo, torch.maximum(spans[..., 1].clamp(max=cut), lo + 1)], -1).to(torch.int32).to(DEV)
        base = _span_launch(qkv_d, clipped, B, H, N)
        dirty = qkv.view(B, N, 3 * C).clone()
        dirty[:, cut:, C:] = (1.0e4 * torch.randn(B, N - cut, 2 * C, generator=gen)).to(BF)
        assert torch.equal(_span_launch(dirty.view(B * N, 3 * C).to(DEV), clipped, B, H, N), base), "a key outside every span reached the output"


@pytest.mark.parametrize("N,kind", [(N, kind) for N in (17, 65, 129, 256) for kind in ("partition", "midtile") if kind != "midtile" or N >= 128])
def test_span_and_byte_mask_attention_are_one_kernel_body(N, kind):
    """Spans s and the dense mask spans_to_mask(s), expanded to [B*H, N, N], are two mask policies of ONE kernel body (csrc/attn_short.hpp): the
    outputs are bit-identical.  A span window starts on a multiple of 64, so a lane owns the same keys under both policies; a masked key adds an
    exact zero to the row sum and to O; 64-key tiles and fragment pairs line up.  (`midtile` needs two key tiles: N >= 128, as in _SPAN_CASES.)"""
    B, H = 2, 3
    gen = torch.Generator().manual_seed(7000 + 10 * N + len(kind))
    qkv_d = torch.randn(B * N, 3 * H * 64, generator=gen).to(BF).to(DEV)
    spans = _layout(kind, B, N, gen)
    dense_d = R.spans_to_mask(spans)[:, None].expand(B, H, N, N).reshape(B * H, N, N).to(torch.uint8).contiguous().to(DEV)
    by_span = _span_launch(qkv_d, spans.to(torch.int32).to(DEV), B, H, N)
    by_mask = _span_launch(qkv_d, None, B, H, N, dense_d=dense_d)
    assert torch.equal(by_span, by_mask), f"{int((by_span != by_mask).sum())} elements differ between the span and the byte-mask policy"


def test_span_attention_refusals():
    from anyedit_amd import ops
    x = torch.zeros(16, 192, dtype=BF, device=DEV)
    sp = torch.zeros(1, 16, 2, dtype=torch.int32, device=DEV)
    st = (16 * 192, 64, 192)
    with pytest.raises(ValueError, match="head_dim"):
        ops.attention_span_short(x, x, x, sp, 1, 1, 16, 32, 1.0, st, st, st)
    with pytest.raises(ValueError, match="sequence length"):
        ops.attention_span_short(x, x, x, sp, 1, 1, 257, 64, 1.0, st, st, st)
    with pytest.raises(ValueError, match="spans"):
        ops.attention_span_short(x, x, x, sp[:, :8], 1, 1, 16, 64, 1.0, st, st, st)


# ------------------------------------------------------------------------------------------------------------ spans, position ids, dense mask
def _check_spans(ids, dtype):
    from anyedit_amd import ops
    want_s, want_p = R.text_spans(ids, SPECIAL)
    spans, pos, dense = ops.gdino_text_spans(ids.to(dtype).to(DEV), SPECIAL, want_mask=True)
    assert spans.dtype == torch.int32 and pos.dtype == torch.int64 and dense.dtype == torch.bool
    assert torch.equal(spans.cpu().long(), want_s) and torch.equal(pos.cpu(), want_p)
    assert torch.equal(dense.cpu(), R.spans_to_mask(want_s)), "the dense mask is the spans' expansion"
    s2, p2, none = ops.gdino_text_spans(ids.to(dtype).to(DEV), SPECIAL)
    assert none is None and torch.equal(s2, spans) and torch.equal(p2, pos)
    return spans, pos, dense


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_text_spans_reproduce_the_reference_fixture(dtype):
    o = R.stored("a")
    _, pos, dense = _check_spans(T(o["input_ids"]), dtype)
    assert torch.equal(pos.cpu(), T(o["position_ids"])) and torch.equal(dense.cpu(), T(o["mask"]))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shape", [(4, 256), (3, 1), (2, 65)])
def test_text_spans_vs_the_restated_rule(shape, dtype):
    gen = torch.Generator().manual_seed(shape[1])
    ids = torch.randint(0, 30, shape, generator=gen)
    ids[:, 0] = 1
    if shape[1] > 8:
        ids[0, -1] = 2            # a special token on the last column
        ids[1, -1] = 20           # and a row without one
        ids[1, -40:] = 0          # a long padding tail
    _check_spans(ids, dtype)


def test_mask_generators_keep_the_reference_signatures():
    from anyedit_amd.groundingdino.bertwarper import generate_masks_with_special_tokens, generate_masks_with_special_tokens_and_transfer_map
    o = R.stored("a")
    tok = {"input_ids": T(o["input_ids"]).to(DEV)}
    mask, pos = generate_masks_with_special_tokens(tok, SPECIAL, None)
    assert mask.dtype == torch.bool and pos.dtype == torch.long
    assert torch.equal(mask.cpu(), T(o["mask"])) and torch.equal(pos.cpu(), T(o["position_ids"]))
    mask2, pos2, c2t = generate_masks_with_special_tokens_and_transfer_map(tok, SPECIAL, None)
    assert torch.equal(mask2, mask) and torch.equal(pos2, pos) and len(c2t) == 4
    for b, c in enumerate(c2t):
        assert c.dtype == torch.bool and torch.equal(c.cpu(), T(o[f"c2t.{b}"])), b


# ------------------------------------------------------------------------------------------------------------ embeddings + LayerNorm
@pytest.mark.parametrize("C", [128, 768])
@pytest.mark.parametrize("nulls", [False, True])
def test_embed_layernorm_vs_float64(C, nulls):
    """LayerNorm(word + position + token_type) on the bf16 tables against float64, every element under tests/norm_ref.py's LayerNorm bound
    (groups = 1, two-pass statistics); ids and positions outside their tables land on the tables' edge rows."""
    from anyedit_amd import ops
    gen = torch.Generator().manual_seed(C + nulls)
    B, N, V, P, TY = 3, 17, 50, 40, 2
    word, ptab, ttab = ((s * torch.randn(n, C, generator=gen)).to(BF) for n, s in ((V, 1.0), (P, 0.5), (TY, 2.0)))
    gamma, beta = norm_ref.make_affine(gen, C)
    ids = torch.randint(0, V, (B, N), generator=gen)
    pids = torch.randint(0, P, (B, N), generator=gen)
    tids = torch.randint(0, TY, (B, N), generator=gen)
    ids[0, 0], ids[0, 1], ids[2, 16] = -5, 1000, V
    pids[1, 0], pids[1, 1], tids[2, 0] = -1, 99, 7
    d = lambda t: t.to(DEV)
    buf = torch.full((B * N * C + 2 * GUARD,), SENTINEL, dtype=BF, device=DEV)
    out = buf[GUARD:GUARD + B * N * C].view(B * N, C)
    ops.bert_embed_ln(d(ids), d(word), d(ptab), d(ttab), d(gamma), d(beta), 1e-12, position_ids=None if nulls else d(pids),
                      type_ids=None if nulls else d(tids), out=out)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    pp = torch.arange(N).expand(B, N) if nulls else pids.clamp(0, P - 1)
    tt = torch.zeros(B, N, dtype=torch.long) if nulls else tids.clamp(0, TY - 1)
    x = word.to(F64)[ids.clamp(0, V - 1)] + ptab.to(F64)[pp] + ttab.to(F64)[tt]
    r = norm_ref.forward(x.view(B * N, 1, C), gamma, beta, 1, 1e-12, 0, False)
    ratio = float(((out.cpu().to(F64).view(B * N, 1, C) - r["y"]).abs() / r["bnd"]).max())
    print(f"embed + LayerNorm C={C} nulls={nulls}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ tiny towers vs golden
def _judge(name, hip, ctl, ref, report):
    e_hip, e_ctl = rel_l2(hip.float().cpu(), ref), rel_l2(ctl, ref)
    report.append(f"{name}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
    return e_hip <= 1.5 * e_ctl


def _tokenized(geom, device="cpu"):
    o = R.stored(geom)
    return {k: T(o[k]).to(device) for k in ("input_ids", "attention_mask", "token_type_ids")}


@pytest.mark.parametrize("geom", R.GEOMS)
def test_tiny_tower_vs_transformers_golden(geom):
    """Every stored output of the fixture: err(HIP) <= 1.5 x err(control), control = bert_ref(bf16_storage=True) on the same weights.  The
    sub-sentence route (span kernel), the same masks as a dense 3-D mask (the general route) and the 2-D padding mask."""
    from anyedit_amd import ops
    o, sd, H = R.stored(geom), R.weights(geom), R.config(geom)["num_attention_heads"]
    tok = _tokenized(geom)
    ids, amask, tids = tok["input_ids"], tok["attention_mask"], tok["token_type_ids"]
    mask, pos = T(o["mask"]), T(o["position_ids"])
    m = R.module(geom, DEV)
    ctl = R.bert_forward(sd, ids, H, allowed=mask, position_ids=pos, token_type_ids=tids, prefix="bert.", bf16_storage=True)
    ctl_p = R.bert_forward(sd, ids, H, allowed=amask.bool(), token_type_ids=tids, prefix="bert.", bf16_storage=True)
    report, ok = [], True
    with torch.no_grad():
        spans, _, _ = ops.gdino_text_spans(ids.to(DEV), SPECIAL)
        out = m.bert(input_ids=ids, token_type_ids=tids, position_ids=pos, key_spans=spans, output_hidden_states=True)
        assert len(out.hidden_states) == len(ctl["hidden_states"]) and out[0] is out.last_hidden_state and out[1] is out.pooler_output
        for i, h in enumerate(out.hidden_states):
            ok &= _judge(f"{geom} hidden_states[{i}]", h, ctl["hidden_states"][i], T(o[f"hs.{i}"]), report)
        ok &= _judge(f"{geom} last_hidden_state", out.last_hidden_state, ctl["last_hidden_state"], T(o["last_hidden_state"]), report)
        ok &= _judge(f"{geom} pooler_output", out.pooler_output, ctl["pooler_output"], T(o["pooler_output"]), report)
        td = m.encode_tokenized(tok)
        ok &= _judge(f"{geom} feat_map", td["encoded_text"], R.feat_map(sd, ctl["last_hidden_state"], bf16_storage=True), T(o["feat_map"]), report)
        assert td["encoded_text"].dtype == BF and td["text_token_mask"].dtype == torch.bool and td["text_self_attention_masks"].dtype == torch.bool
        assert torch.equal(td["text_self_attention_masks"].cpu(), mask) and torch.equal(td["position_ids"].cpu(), pos)
        assert torch.equal(td["text_token_mask"].cpu(), amask.bool())
        dense = m.bert(input_ids=ids, token_type_ids=tids, position_ids=pos, attention_mask=mask)          # the general route on the same masks
        ok &= _judge(f"{geom} last_hidden_state (3-D mask route)", dense.last_hidden_state, ctl["last_hidden_state"], T(o["last_hidden_state"]), report)
        plain = m.bert(input_ids=ids, token_type_ids=tids, attention_mask=amask, output_hidden_states=True)  # the 2-D mask route
        for i, h in enumerate(plain.hidden_states):
            ok &= _judge(f"{geom} plain hidden_states[{i}]", h, ctl_p["hidden_states"][i], T(o[f"plain.hs.{i}"]), report)
        ok &= _judge(f"{geom} plain pooler_output", plain.pooler_output, ctl_p["pooler_output"], T(o["plain.pooler_output"]), report)
        m2 = R.module(geom, DEV, sub_sentence_present=False)
        td2 = m2.encode_tokenized(tok)
        ok &= _judge(f"{geom} plain feat_map", td2["encoded_text"], R.feat_map(sd, ctl_p["last_hidden_state"], bf16_storage=True), T(o["plain.feat_map"]), report)
        assert torch.equal(td2["text_self_attention_masks"].cpu(), mask) and torch.equal(td2["position_ids"].cpu(), pos)
    print("\n".join(report))
    assert ok, "\n".join(report)


def test_truncation_at_max_text_len():
    """groundingdino.py:245-252 with max_text_len = 13 < N = 21: the masks and position ids are the full ones cut, the encoder runs on 13 tokens."""
    geom, K = "a", 13
    o, sd, H = R.stored(geom), R.weights(geom), R.config(geom)["num_attention_heads"]
    tok = _tokenized(geom)
    mask, pos = T(o["mask"])[:, :K, :K], T(o["position_ids"])[:, :K]
    m = R.module(geom, DEV, max_text_len=K)
    with torch.no_grad():
        td = m.encode_tokenized(tok)
    assert tuple(td["encoded_text"].shape) == (4, K, 256) and tuple(td["text_token_mask"].shape) == (4, K)
    assert torch.equal(td["text_self_attention_masks"].cpu(), mask) and torch.equal(td["position_ids"].cpu(), pos)
    assert torch.equal(td["text_token_mask"].cpu(), tok["attention_mask"][:, :K].bool())
    kw = dict(allowed=mask, position_ids=pos, token_type_ids=tok["token_type_ids"][:, :K], prefix="bert.")
    ref = R.feat_map(sd, R.bert_forward(sd, tok["input_ids"][:, :K], H, **kw)["last_hidden_state"])
    ctl = R.feat_map(sd, R.bert_forward(sd, tok["input_ids"][:, :K], H, bf16_storage=True, **kw)["last_hidden_state"], bf16_storage=True)
    report = []
    ok = _judge("truncated feat_map", td["encoded_text"], ctl, ref, report)
    print(report[0])
    assert ok, report[0]


# ------------------------------------------------------------------------------------------------------------ full size
BASE = dict(vocab_size=1024, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=512,
            type_vocab_size=2)


def _base_ids():
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(10, 1024, (2, 256), generator=gen)
    ids[0, 0], ids[0, 255] = 1, 2
    ids[0, torch.tensor([5, 6, 30, 63, 64, 100, 101, 128, 200, 254])] = torch.tensor([3, 3, 4, 3, 3, 3, 4, 3, 3, 3])
    ids[1] = 0
    ids[1, :9] = torch.tensor([1, 500, 3, 600, 601, 3, 700, 3, 2])       # "cat . red chair . dog ." -like: a 9-token caption padded out
    return ids


def test_full_size_tower_vs_restatement():
    """BERT-base geometry (word table cut to 1024 rows), seeded weights, B = 2, N = 256, one row a 9-token caption padded out: HIP vs
    bert_ref fp32 under the 1.5 x control rule (the control's own rel-L2 at this geometry on a CPU run with this seed: last_hidden_state
    1.11e-2, feat_map 1.13e-2)."""
    from anyedit_amd.checkpoints import load_groundingdino_text
    from anyedit_amd.groundingdino.groundingdino import GroundingDINOText
    sd = R.seeded_state_dict(BASE, 256, seed=3)
    ids = _base_ids()
    tok = {"input_ids": ids, "attention_mask": (ids != 0).long(), "token_type_ids": torch.zeros_like(ids)}
    spans, pos = R.text_spans(ids, SPECIAL)
    kw = dict(allowed=R.spans_to_mask(spans), position_ids=pos, prefix="bert.")
    ref = R.bert_forward(sd, ids, 12, **kw)["last_hidden_state"]
    ctl = R.bert_forward(sd, ids, 12, bf16_storage=True, **kw)["last_hidden_state"]
    m = GroundingDINOText(BASE, hidden_dim=256, special_token_ids=SPECIAL)
    load_groundingdino_text(m, sd)
    m = m.eval().requires_grad_(False).to(DEV)
    report = []
    with torch.no_grad():
        td = m.encode_tokenized(tok)
        last = m.bert(input_ids=ids, position_ids=td["position_ids"], key_spans=spans.to(torch.int32).to(DEV), output_pooler=False).last_hidden_state
        ok = _judge("BERT-base last_hidden_state", last, ctl, ref, report)
        ok &= _judge("BERT-base feat_map", td["encoded_text"], R.feat_map(sd, ctl, bf16_storage=True), R.feat_map(sd, ref), report)
    assert torch.equal(td["position_ids"].cpu(), pos) and torch.equal(td["text_self_attention_masks"].cpu(), R.spans_to_mask(spans))
    print("\n".join(report))
    assert ok, "\n".join(report)


# ------------------------------------------------------------------------------------------------------------ graph, allocations
def test_encode_is_capturable_and_allocates_nothing_after_the_first_call():
    m = R.module("a", DEV)
    tok = _tokenized("a", DEV)
    tok["attention_mask"] = tok["attention_mask"].bool()
    with torch.no_grad():
        first = {k: v.clone() for k, v in m.encode_tokenized(tok).items()}
        m.encode_tokenized(tok)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        third = m.encode_tokenized(tok)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        assert after == before, f"{after - before} allocations in the third encode"
        assert all(torch.equal(third[k], first[k]) for k in first)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.encode_tokenized(tok)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.encode_tokenized(tok)
        new = {k: v.flip(0).contiguous() for k, v in tok.items()}      # other captions in the captured buffers
        for k in tok:
            tok[k].copy_(new[k])
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        eager = {k: v.clone() for k, v in m.encode_tokenized(new).items()}
    for k in eager:
        assert torch.equal(replayed[k], eager[k]), f"graph replay differs from the eager encode: {k}"
    assert not torch.equal(replayed["encoded_text"], first["encoded_text"])


# ------------------------------------------------------------------------------------------------------------ plug-in
def test_text_dict_goes_straight_into_the_transformer():
    import gdino_dec_ref as D
    io = D.tower_io()
    srcs, masks, poss, _, _ = D.tower_inputs(io)
    bs = srcs[0].shape[0]
    tower = D.tower_module("standard", DEV)
    m = R.module("a", DEV)
    tok = {k: v[:bs].contiguous() for k, v in _tokenized("a").items()}
    d = lambda t: t.to(DEV)
    with torch.no_grad():
        td = m.encode_tokenized(tok)
        assert sorted(td) == ["encoded_text", "position_ids", "text_self_attention_masks", "text_token_mask"] and td["encoded_text"].shape[-1] == D.GEOM["d_model"]
        hs, refs, hs_enc, ref_enc, ibp = tower([d(s) for s in srcs], [d(k) for k in masks], None, [d(p) for p in poss], None, None, td)
    torch.cuda.synchronize()
    nq = D.GEOM["num_queries"]
    assert len(hs) == D.GEOM["num_decoder_layers"] and all(tuple(h.shape) == (bs, nq, 256) and bool(torch.isfinite(h.float()).all()) for h in hs)
    assert all(tuple(r.shape) == (bs, nq, 4) and bool(torch.isfinite(r).all()) for r in refs)
    assert tuple(td["encoded_text"].shape) == (bs, 21, 256) and bool(torch.isfinite(td["encoded_text"].float()).all())
