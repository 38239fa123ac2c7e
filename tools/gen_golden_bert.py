"""Fixture generator for GroundingDINO's text side: tests/golden/bert_tiny_*.npz.

Runs on a development machine only (it needs `transformers`; the tests read only the .npz files).  Two sources, neither copied into this tree:
  * the sub-sentence masks, position ids and cate_to_token masks come from the reference's own `generate_masks_with_special_tokens` /
    `generate_masks_with_special_tokens_and_transfer_map`, loaded from `models/GroundingDINO/bertwarper.py` BY FILE PATH (pass the reference
    checkout with --reference or ANYEDIT_REFERENCE).  `transformers` is imported FIRST and only then inert stubs for `torchvision` /
    `torchvision.ops.boxes` (the file imports `nms`, unused here) go into `sys.modules`; the other order breaks transformers' own import.
  * the encoder outputs come from `transformers.BertModel`.  The reference's `BertModelWarper.forward` is a copy of an old BertModel.forward that
    lets a 3-D [B, N, N] mask through; it does not run under current transformers (`get_head_mask` is gone).  The installed BertModel refuses a
    3-D mask but takes a 4-D one [B, 1, N, N] as it is.  It must be the ADDITIVE form (0 = allowed, -inf = not: what the reference's
    `get_extended_attention_mask` makes of the 3-D mask): eager attention ADDS the mask to the logits, so a bool `mask[:, None]` would add
    1.0 / 0.0 and mask nothing (sdpa does take a bool mask; with the additive form eager and sdpa agree to 1e-7).  The stored outputs are
    `BertModel(input_ids, attention_mask=additive(mask)[:, None], position_ids, token_type_ids)` with eager attention.
Chain of trust: reference + transformers produce the stored values -> tests/bert_ref.py, a plain-torch restatement, is pinned to them at
rel-L2 <= 1e-5 by the CPU suite -> the GPU suite trusts the restatement at sizes no fixture could hold.

Two geometries, both head_dim 64 (BERT's):
  a   hidden 128, 2 heads, 2 layers, intermediate 512
  b   hidden 192, 3 heads (an odd head count, as BERT's 12 is not a power of two), 1 layer, intermediate 768
Both: vocab 64, 64 positions, 2 token types, feat_map to 256; B = 4, N = 21; special ids [CLS] 1, [SEP] 2, "." 3, "?" 4, padding 0.  Rows:
  0  several phrases, a "?", a one-token phrase, two adjacent special tokens, [SEP] in the interior and a padding tail
  1  a short row: one phrase, [SEP], sixteen padding tokens
  2  a row that fills N ([SEP] on the last column, so the tokens of the last phrase attend themselves only)
  3  a long phrase, a "?", two adjacent [SEP], padding; token type 1 from column 10 on
What the default init hides is re-drawn: LayerNorm weights U(0.5, 1.5) and biases N(0, 0.1^2), every Linear bias N(0, 0.1^2), matrices
U(-a, a) with a = sqrt(3 / fan_in) (query / key x 2), embedding tables N(0, 0.05^2).  Every weight is rounded to bf16 BEFORE the model runs.

Files (none may pass the repository's 1 MiB limit), per geometry <g>:
  bert_tiny_<g>_w<i>.npz   w.<key>: a slice of the state dict (`bert.*`, `feat_map.*`) as bf16 bits (int16); the slices are cut by size
  bert_tiny_<g>_io.npz     input_ids, attention_mask, token_type_ids, special_ids; mask / position_ids / c2t.<b> (the reference's); hs.<i>,
                           last_hidden_state, pooler_output, feat_map (sub-sentence masks); plain.* (the same under the 2-D padding mask:
                           sub_sentence_present=False); keys = the sorted state-dict key names; config.<name> integers
"""
import argparse
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOMS = {
    "a": dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512),
    "b": dict(hidden_size=192, num_attention_heads=3, num_hidden_layers=1, intermediate_size=768),
}
COMMON = dict(vocab_size=64, max_position_embeddings=64, type_vocab_size=2)
HIDDEN_DIM = 256
SPECIAL = [1, 2, 3, 4]
W_FILE_BYTES = 900 * 1024
ROWS = [
    [1, 10, 11, 3, 12, 13, 14, 3, 15, 4, 16, 3, 3, 17, 18, 3, 2, 0, 0, 0, 0],
    [1, 20, 21, 3, 2] + [0] * 16,
    [1, 22, 23, 24, 3, 25, 26, 3, 27, 28, 29, 30, 3, 31, 4, 32, 33, 34, 35, 3, 2],
    [1, 40, 41, 42, 43, 44, 45, 46, 47, 3, 48, 49, 4, 2, 2, 0, 0, 0, 0, 0, 0],
]


def load_reference(root):
    """The reference's bertwarper module, loaded by path; transformers first, then the torchvision stubs."""
    import transformers  # noqa: F401
    if "torchvision" not in sys.modules:
        boxes = types.ModuleType("torchvision.ops.boxes")
        boxes.nms = None
        opsm = types.ModuleType("torchvision.ops")
        opsm.boxes = boxes
        tv = types.ModuleType("torchvision")
        tv.ops = opsm
        sys.modules.update({"torchvision": tv, "torchvision.ops": opsm, "torchvision.ops.boxes": boxes})
    path = os.path.join(root, "GroundingDINO", "groundingdino", "models", "GroundingDINO", "bertwarper.py")
    spec = importlib.util.spec_from_file_location("reference_bertwarper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def redraw(m, g):
    norms = {k for k, mod in m.named_modules() if isinstance(mod, torch.nn.LayerNorm)}
    embeds = {k for k, mod in m.named_modules() if isinstance(mod, torch.nn.Embedding)}
    with torch.no_grad():
        for k, v in m.named_parameters():
            owner, leaf = k.rsplit(".", 1)
            if owner in norms:
                v.copy_(0.5 + torch.rand(v.shape, generator=g) if leaf == "weight" else 0.1 * torch.randn(v.shape, generator=g))
            elif owner in embeds:
                v.copy_(0.05 * torch.randn(v.shape, generator=g))
            elif v.dim() == 2:
                a = math.sqrt(3.0 / v.shape[1]) * (2.0 if owner.endswith((".query", ".key")) else 1.0)
                v.copy_((2 * torch.rand(v.shape, generator=g) - 1) * a)
            else:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            v.copy_(v.bfloat16().float())         # stored as bf16 bit patterns; the model runs on these values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ANYEDIT_REFERENCE"), help="checkout of the reference project (AnyEdit)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference <AnyEdit checkout> (or set ANYEDIT_REFERENCE)")
    ref = load_reference(args.reference)
    from transformers import BertConfig, BertModel
    import bert_ref as R
    rel = lambda a, b: float((a.detach().double() - b.detach().double()).norm() / b.detach().double().norm())
    bits = lambda v: v.detach().bfloat16().view(torch.int16).numpy()

    ids = torch.tensor(ROWS)
    B, N = ids.shape
    amask = (ids != 0).long()
    tids = torch.zeros_like(ids)
    tids[3, 10:] = 1
    tokenized = {"input_ids": ids, "attention_mask": amask, "token_type_ids": tids}
    mask, pos = ref.generate_masks_with_special_tokens(tokenized, SPECIAL, None)
    mask2, pos2, c2t = ref.generate_masks_with_special_tokens_and_transfer_map(tokenized, SPECIAL, None)
    assert torch.equal(mask, mask2) and torch.equal(pos, pos2)
    spans, rpos = R.text_spans(ids, SPECIAL)
    print("span rule vs reference: mask equal", bool(torch.equal(R.spans_to_mask(spans), mask)), "position ids equal", bool(torch.equal(rpos, pos)),
          "cate_to_token equal", all(torch.equal(a, b) for a, b in zip(R.cate_to_token(ids, SPECIAL), c2t)))

    for seed, (name, geom) in enumerate(GEOMS.items()):
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(700 + seed)
        cfg = BertConfig(**geom, **COMMON, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12,
                         attn_implementation="eager")
        m = BertModel(cfg).eval()
        fm = torch.nn.Linear(geom["hidden_size"], HIDDEN_DIM)
        redraw(m, g)
        redraw(torch.nn.ModuleDict({"feat_map": fm}), g)
        sd = {"bert." + k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith(("position_ids", "token_type_ids"))}
        sd.update({"feat_map." + k: v.detach().clone() for k, v in fm.state_dict().items()})
        files, cur, size = [], {}, 0
        for k in sorted(sd):
            n = sd[k].numel() * 2
            if cur and size + n > W_FILE_BYTES:
                files.append(cur)
                cur, size = {}, 0
            cur["w." + k] = bits(sd[k])
            size += n
        files.append(cur)
        for i, f in enumerate(files):
            np.savez_compressed(os.path.join(OUT, f"bert_tiny_{name}_w{i}.npz"), **f)

        with torch.no_grad():
            additive = torch.zeros(B, 1, N, N).masked_fill(~mask[:, None], float("-inf"))
            sub = m(input_ids=ids, attention_mask=additive, position_ids=pos, token_type_ids=tids, output_hidden_states=True)
            plain = m(input_ids=ids, attention_mask=amask, token_type_ids=tids, output_hidden_states=True)
            o = dict(input_ids=ids.numpy(), attention_mask=amask.numpy(), token_type_ids=tids.numpy(), special_ids=np.array(SPECIAL),
                     mask=mask.numpy(), position_ids=pos.numpy(), keys=np.array(sorted(sd)))
            for b, c in enumerate(c2t):
                o[f"c2t.{b}"] = c.numpy()
            for tag, r in (("", sub), ("plain.", plain)):
                for i, h in enumerate(r.hidden_states):
                    o[f"{tag}hs.{i}"] = h.numpy()
                o[tag + "last_hidden_state"] = r.last_hidden_state.numpy()
                o[tag + "pooler_output"] = r.pooler_output.numpy()
                o[tag + "feat_map"] = fm(r.last_hidden_state).numpy()
            for k, v in {**geom, **COMMON, "hidden_dim": HIDDEN_DIM}.items():
                o["config." + k] = np.array(v)
        assert all(np.isfinite(v).all() for k, v in o.items() if v.dtype.kind == "f")
        np.savez_compressed(os.path.join(OUT, f"bert_tiny_{name}_io.npz"), **o)

        H = geom["num_attention_heads"]
        mine = R.bert_forward(sd, ids, H, allowed=mask, position_ids=pos, token_type_ids=tids, prefix="bert.")
        mine2 = R.bert_forward(sd, ids, H, allowed=amask.bool(), token_type_ids=tids, prefix="bert.")
        print(f"{name}: restatement vs transformers rel-L2: last {rel(mine['last_hidden_state'], sub.last_hidden_state):.2e} "
              f"pooler {rel(mine['pooler_output'], sub.pooler_output):.2e} feat_map {rel(R.feat_map(sd, mine['last_hidden_state']), fm(sub.last_hidden_state)):.2e} "
              f"plain last {rel(mine2['last_hidden_state'], plain.last_hidden_state):.2e}")
    for f in sorted(os.listdir(OUT)):
        if f.startswith("bert_tiny"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
