"""GPU tests of the GroundingDINO detector (anyedit_amd/groundingdino/groundingdino.py, inference.py) at the tiny geometry of
tests/gdino_model_ref.py: two images of 50x38 and 40x40 padded to 50x40 (a real padding mask, ragged 7x5 / 4x3 stage maps, a 2x2 stride-2
level), B = 2, the stand-in tokenizer.

The tower rule of the project: rel-L2 of every compared tensor against the fp32 restatement is at most 1.5 x that of the bf16-storage control
(the same restatement, rounded to bf16 wherever the HIP path stores bf16).  The query selection is forced through `topk_proposals` from the
reference side, as the decoder tests do, so that both sides decode the same rows; a second case lets it run free.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gdino_dec_ref as DR  # noqa: E402
import gdino_model_ref as MR  # noqa: E402
import gdino_neck_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIAL = [1, 2, 3, 4]
_CACHE = {}


def _model():
    if "m" not in _CACHE:
        _CACHE["m"] = MR.tiny_model(DEV)
    return _CACHE["m"]


def _refs():
    """(fp32 restatement, bf16-storage control with the restatement's selection), computed once"""
    if "ref" not in _CACHE:
        px, mask, _, tok = MR.tiny_inputs()
        sd = MR.tiny_state_dict()
        ref = MR.model_forward(sd, px, mask, tok["input_ids"], tok["attention_mask"], SPECIAL, MR.bert_config()["num_attention_heads"])
        ctl = MR.model_forward(sd, px, mask, tok["input_ids"], tok["attention_mask"], SPECIAL, MR.bert_config()["num_attention_heads"], store=DR.round_bf16,
                               topk_proposals=ref["topk_proposals"])
        _CACHE["ref"] = (ref, ctl)
    return _CACHE["ref"]


def _run(forced):
    m = _model()
    _, _, imgs, _ = MR.tiny_inputs()
    ref, _ = _refs()
    idx = ref["topk_proposals"].to(DEV) if forced else None
    with torch.no_grad():
        out = m([im.to(DEV) for im in imgs], captions=MR.CAPTIONS, topk_proposals=idx)
    torch.cuda.synchronize()
    got = {k: v.float().cpu() for k, v in out.items()}
    got.update(src_flatten=m.last_src_flatten.float().cpu(), pos_flatten=m.last_pos_flatten.float().cpu(), mask_flatten=m.last_mask_flatten.cpu(),
               topk_logits=m.transformer.last_topk_logits.float().cpu(), selected=m.transformer.last_topk_proposals.cpu())
    return got


def _rel_fin(a, b):
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), "the -inf pattern differs"
    a, b = a.double()[fin], b.double()[fin]
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_model_with_forced_selection_under_the_tower_rule():
    ref, ctl = _refs()
    got = _run(forced=True)
    assert torch.equal(got["mask_flatten"], ref["mask_flatten"]), "mask_flatten"
    assert bool(ref["mask_flatten"].any()) and not bool(ref["mask_flatten"].all(1).any()), "the case must hold a real padding mask"
    assert torch.equal(torch.isneginf(got["pred_logits"]), torch.isneginf(ref["pred_logits"])), "the -inf pattern of pred_logits"
    report, ok = [], True
    for k in ("pred_logits", "pred_boxes", "src_flatten", "pos_flatten"):
        e_hip, e_ctl = _rel_fin(got[k], ref[k]), _rel_fin(ctl[k], ref[k])
        report.append(f"{k}: HIP {e_hip:.3e}  control {e_ctl:.3e}  ratio {e_hip / max(e_ctl, 1e-30):.2f}")
        ok &= e_hip <= 1.5 * e_ctl
    print("\n".join(report))
    assert ok, "\n".join(report)


def test_model_with_free_selection():
    """The selection is the stable top-k of the model's own scores; against the reference's scores it may differ only on rows whose gap to the
    k-th score is below twice the control's largest score deviation."""
    ref, ctl = _refs()
    forced, free = _run(forced=True), _run(forced=False)
    nq = DR.GEOM["num_queries"]
    ref_s = ref["topk_logits"]
    e = float((ctl["topk_logits"] - ref_s).abs().max())
    sel = free["selected"]
    assert torch.equal(sel, DR.stable_topk(free["topk_logits"], nq)), "the selection is not the stable sort of the model's own scores"
    s_k = torch.sort(ref_s, 1, descending=True)[0][:, nq - 1]
    for b in range(sel.shape[0]):
        chosen = torch.zeros(ref_s.shape[1], dtype=torch.bool)
        chosen[sel[b]] = True
        assert bool((ref_s[b][sel[b]] >= s_k[b] - 2 * e).all()), "a selected row scores below the k-th reference score by more than 2e"
        assert bool(chosen[ref_s[b] > s_k[b] + 2 * e].all()), "a row above the k-th reference score by more than 2e is not selected"
    same = torch.equal(sel, ref["topk_proposals"])
    print(f"free selection: e = {e:.3e}, indices equal to the reference's: {same}")
    if same:
        for k in ("pred_logits", "pred_boxes"):
            assert torch.equal(forced[k], free[k]), k


def test_model_graph_capture_replays_the_eager_result():
    m = _model()
    px, mask, _, tok = MR.tiny_inputs()
    ref, _ = _refs()
    dpx, dmask, idx = px.to(DEV), mask.to(DEV), ref["topk_proposals"].to(DEV)
    dtok = {k: v.to(DEV) for k, v in tok.items()}
    dtok["attention_mask"] = dtok["attention_mask"].bool()

    def fwd():
        out = m.detect(dpx, dmask, dtok, topk_proposals=idx)
        return out["pred_logits"], out["pred_boxes"]

    eager = [t.clone() for t in fwd()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd()                                   # warm the allocator and the caches on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = fwd()
        for t in outs:
            t.zero_()
        g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8)), "the replay differs from the eager forward"


def test_get_grounding_output_end_to_end():
    """inference.get_grounding_output on the tiny model against the CPU statement of tools/tool.py:125-147 applied to the same pred_logits and
    pred_boxes; the thresholds sit in the widest gaps of the model's own probabilities, so neither side decides on a rounding."""
    from anyedit_amd.groundingdino import inference as I
    m = _model()
    _, _, imgs, _ = MR.tiny_inputs()
    caption = "  Cat . Red dog ."
    cap = I.preprocess_caption(caption)
    assert cap == "cat . red dog ."
    with torch.no_grad():
        out = m(imgs[0][None].to(DEV), captions=[cap])
    logits, boxes = out["pred_logits"][0].cpu(), out["pred_boxes"][0].cpu()
    p = logits.sigmoid()
    s = p.max(1)[0].sort()[0]
    i = int((s[1:] - s[:-1]).argmax())
    box_t = float((s[i] + s[i + 1]) / 2)
    v = p[p > 0].flatten().sort()[0]
    j = int((v[1:] - v[:-1]).argmax())
    text_t = float((v[j] + v[j + 1]) / 2)
    assert float((p - box_t).abs().min()) >= 1e-5 and float((p - text_t).abs().min()) >= 1e-5, "a sigmoid lies within 1e-5 of a threshold"
    ri, rs, rb, rp = NR.ground(logits, boxes, box_t, text_t)
    assert 0 < ri.numel() < logits.shape[0]
    tok = m.tokenizer
    tokenized = tok(cap)
    names = [I.get_phrases_from_posmap(pm, tokenized, tok) for pm in rp]
    got_boxes, got_phrases = I.get_grounding_output(m, imgs[0], caption, box_t, text_t, device=DEV)
    assert got_boxes.device.type == "cpu" and torch.equal(got_boxes, rb)
    assert len(got_phrases) == len(names)
    # The model's own scores are not ours to place: one that lies within 1e-4 of a multiple of 0.01 may truncate to either neighbour, since the
    # device score is within 2^-22 of the host's.  Every other phrase must be the host's string exactly.
    exact = 0
    for got, name, sc in zip(got_phrases, names, rs):
        v = float(sc)
        if abs(v * 100 - round(v * 100)) / 100 >= 1e-4:
            assert got == name + f"({str(v)[:4]})", (got, name, v)
            exact += 1
        else:
            assert got in {name + f"({str(float(torch.tensor(v + d, dtype=torch.float32)))[:4]})" for d in (-2.0 ** -22, 0.0, 2.0 ** -22)}, (got, name, v)
    assert exact > 0
    plain = I.get_grounding_output(m, imgs[0], caption, box_t, text_t, with_logits=False, device=DEV)[1]
    assert plain == names


def test_forward_and_forward_rows_agree_on_the_tower_inputs():
    """Transformer.forward is its flattening followed by forward_rows: the same bits on the decoder golden's inputs, either way in."""
    io = DR.tower_io()
    m = DR.tower_module("standard", DEV)
    srcs, masks, poss, text, tm = DR.tower_inputs(io)
    d = lambda t: t.to(DEV)
    S, K, P, idx = [d(s) for s in srcs], [d(k) for k in masks], [d(p) for p in poss], d(io["topk_proposals"])
    td = lambda: {"encoded_text": d(text), "text_token_mask": d(tm)}
    a = m(S, K, None, P, None, None, td(), topk_proposals=idx)
    src = torch.cat([s.flatten(2).transpose(1, 2) for s in S], 1)
    pos = torch.cat([p.flatten(2).transpose(1, 2) for p in P], 1)
    msk = torch.cat([k.flatten(1) for k in K], 1).contiguous()
    vr = torch.stack([m.get_valid_ratio(k) for k in K], 1)
    b = m.forward_rows(src, msk, pos, [tuple(s.shape[-2:]) for s in S], vr, td(), topk_proposals=idx)
    torch.cuda.synchronize()
    flat = lambda r: [t for part in r for t in (part if isinstance(part, (list, tuple)) else [part])]
    for x, y in zip(flat(a), flat(b)):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
