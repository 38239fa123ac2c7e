"""Host-side checks of GroundingDINO's text side (no GPU): the chain of trust of its fixtures (the restatement against every output
transformers stored, the span rule against the masks the reference's own functions stored), the C ABI's exports and refusals, the checkpoint
loader's three key layouts and its strictness, the constructors' refusals and a stub tokenizer.  Modules are constructed on the CPU: nothing here
launches a kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2, T  # noqa: E402
import bert_ref as R  # noqa: E402


def _inputs(geom):
    o = R.stored(geom)
    return o, T(o["input_ids"]), T(o["attention_mask"]), T(o["token_type_ids"]), [int(t) for t in o["special_ids"]]


def test_fixture_rows_are_what_the_issue_asks_for():
    o, ids, amask, tids, special = _inputs("a")
    assert tuple(ids.shape) == (4, 21) and special == [1, 2, 3, 4]
    s = R.special_mask(ids, special)
    assert bool(s[:, 0].all()), "column 0 of every row is a special token (the reference's contract)"
    assert int((ids[0] == 4).sum()) == 1                                        # a "?"
    assert bool((s[0, 1:] & s[0, :-1]).any())                                   # two adjacent special tokens
    assert ids[0, 10] not in special and bool(s[0, 9]) and bool(s[0, 11])       # a one-token phrase
    assert int(amask[1].sum()) == 5 and int(ids[1, 4]) == 2                     # a short row: [SEP] in the interior, a padding tail
    assert bool(amask[2].all()) and int(ids[2, -1]) == 2                        # a row that fills N
    assert bool(tids.any()) and not bool(tids[:3].any())


@pytest.mark.parametrize("geom", R.GEOMS)
def test_span_rule_reproduces_the_reference_masks(geom):
    o, ids, _, _, special = _inputs(geom)
    spans, pos = R.text_spans(ids, special)
    mask = T(o["mask"])
    assert torch.equal(pos, T(o["position_ids"]))
    assert torch.equal(R.spans_to_mask(spans), mask)
    # every stored mask row is ONE contiguous run of keys, and that run is its [lo, hi): what ae_attn_span_short_bf16 relies on
    B, N = ids.shape
    for b in range(B):
        for n in range(N):
            keys = torch.nonzero(mask[b, n]).flatten()
            assert keys.numel() >= 1 and torch.equal(keys, torch.arange(int(keys[0]), int(keys[-1]) + 1)), (b, n)
            assert (int(keys[0]), int(keys[-1]) + 1) == tuple(spans[b, n].tolist()), (b, n)
    c2t = R.cate_to_token(ids, special)
    for b in range(B):
        assert torch.equal(c2t[b], T(o[f"c2t.{b}"])), b
    from anyedit_amd.groundingdino.bertwarper import cate_to_token_masks
    mine = cate_to_token_masks(R.special_mask(ids, special), spans)
    assert all(torch.equal(a, T(o[f"c2t.{b}"])) for b, a in enumerate(mine))


@pytest.mark.parametrize("geom", R.GEOMS)
def test_restatement_matches_the_transformers_golden(geom):
    """tests/bert_ref.py (fp32) against what transformers' BertModel produced: rel-L2 <= 1e-5, the project's pin for a restatement, on every
    hidden state, last_hidden_state, pooler_output and the feat_map output, under the sub-sentence masks and under the 2-D padding mask."""
    o, ids, amask, tids, _ = _inputs(geom)
    sd, H = R.weights(geom), R.config(geom)["num_attention_heads"]
    runs = {"": R.bert_forward(sd, ids, H, allowed=T(o["mask"]), position_ids=T(o["position_ids"]), token_type_ids=tids, prefix="bert."),
            "plain.": R.bert_forward(sd, ids, H, allowed=amask.bool(), token_type_ids=tids, prefix="bert.")}
    checked = 0
    for tag, r in runs.items():
        got = {f"{tag}hs.{i}": h for i, h in enumerate(r["hidden_states"])}
        got.update({tag + "last_hidden_state": r["last_hidden_state"], tag + "pooler_output": r["pooler_output"],
                    tag + "feat_map": R.feat_map(sd, r["last_hidden_state"])})
        for name, v in got.items():
            e = rel_l2(v, T(o[name]))
            print(f"{geom} {name}: rel-L2 {e:.2e}")
            assert e <= 1e-5, (geom, name, e)
            checked += 1
    assert checked == sum(1 for k in o if k.startswith(("hs.", "plain.")) or k in ("last_hidden_state", "pooler_output", "feat_map")), "every stored output is checked"
    # the two routes differ (the masks matter), and the control is rounding noise and not another function
    assert rel_l2(runs[""]["last_hidden_state"], runs["plain."]["last_hidden_state"]) > 1e-2
    c = R.bert_forward(sd, ids, H, allowed=T(o["mask"]), position_ids=T(o["position_ids"]), token_type_ids=tids, prefix="bert.", bf16_storage=True)
    e = rel_l2(c["last_hidden_state"], runs[""]["last_hidden_state"])
    assert torch.isfinite(c["last_hidden_state"]).all() and 1e-4 < e < 5e-2, e


def test_c_abi_exports_and_refusals():
    """Every refusal happens before any GPU call: this machine has no GPU, and the calls return an argument error with a message."""
    from anyedit_amd import _lib
    L = _lib.lib
    for name in ("ae_gdino_text_spans", "ae_bert_embed_ln_bf16", "ae_attn_span_short_bf16"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    x = torch.zeros(4096, dtype=torch.int64)
    p = x.data_ptr()
    sp = [1, 2, 3, 4, 0, 0, 0, 0]
    assert L.ae_gdino_text_spans(p, 1, 1, 257, 4, *sp, p, p, None, None) == -1 and b"257" in L.ae_last_error()
    assert L.ae_gdino_text_spans(None, 1, 1, 8, 4, *sp, p, p, None, None) == -1 and b"null pointer" in L.ae_last_error()
    assert L.ae_gdino_text_spans(p, 1, 1, 8, 9, *sp, p, p, None, None) == -1 and b"special" in L.ae_last_error()
    st = (0, 64, 64) * 4
    assert L.ae_attn_span_short_bf16(p, p, p, p, p, 1, 1, 257, 64, *st, 0.125, None) == -1 and b"257" in L.ae_last_error()
    assert L.ae_attn_span_short_bf16(p, p, p, p, p, 1, 1, 16, 40, *st, 0.125, None) == -1 and b"head_dim 40" in L.ae_last_error()
    assert L.ae_attn_span_short_bf16(p, p, p, None, p, 1, 1, 16, 64, *st, 0.125, None) == -1 and b"null pointer" in L.ae_last_error()
    assert L.ae_attn_span_short_bf16(p, p, p, p, p, 1, 1, 0, 64, *st, 0.125, None) == -1
    emb = lambda C, ids=p, out=p: L.ae_bert_embed_ln_bf16(ids, None, None, p, p, p, p, p, out, 1, 8, C, 64, 64, 2, 1e-12, None)
    assert emb(100) == -1 and b"multiple of 8" in L.ae_last_error()
    assert emb(4096) == -1 and b"4096" in L.ae_last_error()
    assert emb(128, ids=None) == -1 and b"null pointer" in L.ae_last_error()
    assert L.ae_bert_embed_ln_bf16(p, None, None, p, p, p, p, p, p, 1, 65, 128, 64, 64, 2, 1e-12, None) == -1 and b"position table" in L.ae_last_error()


def test_ops_wrappers_refuse_before_the_library():
    from anyedit_amd import ops
    ids = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gdino_text_spans(ids, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.bert_embed_ln(ids, None, None, None, None, None, 1e-12)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.attention_span_short(torch.zeros(8, 64, dtype=torch.bfloat16), None, None, None, 1, 1, 8, 64, 0.125, (0, 0, 0), (0, 0, 0), (0, 0, 0))


def _tiny(**kw):
    from anyedit_amd.groundingdino.groundingdino import GroundingDINOText
    cfg = dict(R.config("a"))
    hidden_dim = cfg.pop("hidden_dim")
    return GroundingDINOText(cfg, hidden_dim=hidden_dim, special_token_ids=[1, 2, 3, 4], **kw)


def test_loader_accepts_the_three_layouts_and_is_strict():
    from anyedit_amd.checkpoints import load_groundingdino_text
    sd = R.weights("a")
    same = lambda m: all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()) and sorted(m.state_dict()) == sorted(sd)
    m = _tiny()
    assert sorted(m.state_dict()) == [str(k) for k in R.stored("a")["keys"]], "the module's keys are the checkpoint's bert.* and feat_map.*"
    full = dict(sd)
    full.update({"transformer.level_embed": torch.zeros(4, 256), "backbone.0.norm1.weight": torch.zeros(3), "bert.embeddings.position_ids": torch.arange(64)[None]})
    assert load_groundingdino_text(m, full) == "groundingdino" and same(m)
    m = _tiny()
    assert load_groundingdino_text(m, {"model": {"module." + k: v for k, v in full.items()}}) == "groundingdino-module" and same(m)
    m = _tiny()
    bare = {(k[len("bert."):] if k.startswith("bert.") else k): v for k, v in sd.items()}
    bare["embeddings.position_ids"] = torch.arange(64)[None]
    assert load_groundingdino_text(m, bare) == "bert" and same(m)
    for drop in ("bert.encoder.layer.1.output.LayerNorm.bias", "feat_map.weight", "bert.pooler.dense.bias"):
        with pytest.raises(KeyError, match=drop.replace(".", r"\.")):
            load_groundingdino_text(_tiny(), {k: v for k, v in sd.items() if k != drop})
    with pytest.raises(KeyError, match="no place"):
        load_groundingdino_text(_tiny(), dict(sd, **{"bert.encoder.layer.2.output.dense.bias": torch.zeros(128)}))


def test_constructors_and_forward_refuse_what_is_not_built():
    from anyedit_amd.groundingdino.bertwarper import BERT_BASE, BertModel, BertModelWarper
    from anyedit_amd.groundingdino.groundingdino import GroundingDINOText
    assert (BERT_BASE["hidden_size"], BERT_BASE["num_attention_heads"], BERT_BASE["num_hidden_layers"], BERT_BASE["vocab_size"]) == (768, 12, 12, 30522)
    tiny = dict(R.config("a"))
    tiny.pop("hidden_dim")
    for bad, exc in ((dict(is_decoder=True), NotImplementedError), (dict(hidden_act="relu"), NotImplementedError),
                     (dict(position_embedding_type="relative_key"), NotImplementedError), (dict(num_attention_heads=4), ValueError)):
        with pytest.raises(exc):
            BertModel(dict(tiny, **bad))
    m = BertModel(tiny, hidden_dropout_prob=0.1).requires_grad_(False)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    for kw in (dict(head_mask=torch.ones(2)), dict(inputs_embeds=torch.zeros(1, 4, 128)), dict(past_key_values=()), dict(output_attentions=True)):
        with pytest.raises(NotImplementedError):
            m(ids, **kw)
    with pytest.raises(RuntimeError, match="dropout"):
        m.train()(ids)
    with pytest.raises(ValueError, match="GPU only"):
        m.eval()(ids)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m(torch.full((1, 4), 64))
    with pytest.raises(TypeError):
        BertModelWarper(torch.nn.Linear(2, 2))
    w = BertModelWarper(m)
    assert sorted(w.state_dict()) == sorted(m.state_dict()) and w.eval() is w and not m.training and w.train().training and m.training
    with pytest.raises(ValueError, match="tokenizer"):
        GroundingDINOText(tiny)
    with pytest.raises(ValueError, match="max_text_len"):
        GroundingDINOText(tiny, special_token_ids=[1, 2, 3, 4], max_text_len=257)


class StubTokenizer:
    """The Hugging Face call signature over a whitespace vocabulary: [CLS] words [SEP], padded to the longest with 0."""
    VOCAB = {"[PAD]": 0, "[CLS]": 1, "[SEP]": 2, ".": 3, "?": 4, "cat": 10, "dog": 11, "a": 12, "red": 13, "chair": 14}

    def convert_tokens_to_ids(self, tokens):
        return [self.VOCAB[t] for t in tokens]

    def __call__(self, captions, padding="longest", return_tensors="pt"):
        assert padding == "longest" and return_tensors == "pt"
        rows = [[1] + [self.VOCAB[w] for w in c.split()] + [2] for c in captions]
        n = max(len(r) for r in rows)
        ids = torch.tensor([r + [0] * (n - len(r)) for r in rows])
        return {"input_ids": ids, "attention_mask": (ids != 0).long(), "token_type_ids": torch.zeros_like(ids)}


def test_stub_tokenizer_round_trips():
    from anyedit_amd.groundingdino.groundingdino import GroundingDINOText
    tiny = dict(R.config("a"))
    tiny.pop("hidden_dim")
    tok = StubTokenizer()
    m = GroundingDINOText(tiny, hidden_dim=256, tokenizer=tok)
    assert m.specical_tokens == [1, 2, 3, 4] and m.tokenizer is tok
    assert {k.split(".")[0] for k in m.state_dict()} == {"bert", "feat_map"}
    t = tok(["cat . dog .", "a red chair ."])
    assert t["input_ids"].tolist() == [[1, 10, 3, 11, 3, 2], [1, 12, 13, 14, 3, 2]]
    spans, pos = R.text_spans(t["input_ids"], m.specical_tokens)
    assert pos.tolist() == [[0, 0, 1, 0, 1, 0], [0, 0, 1, 2, 3, 0]]
    assert spans[0].tolist() == [[0, 1], [1, 3], [1, 3], [3, 5], [3, 5], [5, 6]]
    with pytest.raises(ValueError, match="GPU only"):
        m.eval()(["cat ."])
