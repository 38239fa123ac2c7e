"""GroundingDINO/groundingdino/models/GroundingDINO/utils.py — the helpers of the feature enhancer, and those of the query selection, the decoder
and the heads on the kernels of csrc/gdino_decoder.hip (`gen_encoder_output_proposals`, `gen_sineembed_for_position`, `MLP`, `ContrastiveEmbed`;
`inverse_sigmoid` of util/misc.py lives here too, where its callers import it from)."""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from anyedit_amd import ops


def _get_clones(module, N, layer_share=False):
    """:16-21: N deep copies (or N references when the layers share weights)."""
    if layer_share:
        return nn.ModuleList([module for _ in range(N)])
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def get_sine_pos_embed(pos_tensor, num_pos_feats=128, temperature=10000, exchange_xy=True):
    """:24-53: pos_tensor [bs, n, k] -> [bs, n, k * num_pos_feats]; per coordinate x, feature 2i is sin(2 pi x / T^(2i/F)) and feature 2i + 1 is
    cos(2 pi x / T^(2i/F)), T = temperature, F = num_pos_feats.  exchange_xy swaps the blocks of the first two coordinates."""
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos_tensor.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    blocks = []
    for j in range(pos_tensor.shape[-1]):
        a = pos_tensor[..., j:j + 1] * (2 * math.pi) / dim_t
        blocks.append(torch.stack((a[..., 0::2].sin(), a[..., 1::2].cos()), dim=3).flatten(2))
    if exchange_xy:
        blocks[0], blocks[1] = blocks[1], blocks[0]
    return torch.cat(blocks, dim=-1)


def _get_activation_fn(activation, d_model=256, batch_dim=0):
    """:188-201.  Only relu is built: it is the epilogue of the feed-forward GEMMs (EPI_RELU), and every GroundingDINO config uses it."""
    if activation == "relu":
        return F.relu
    if activation in ("gelu", "glu", "prelu", "selu"):
        raise NotImplementedError(f"activation {activation!r} is not built on the HIP path: the feed-forward GEMMs carry relu only")
    raise RuntimeError(f"activation should be relu/gelu, not {activation}.")


def inverse_sigmoid(x, eps=1e-3):
    """util/misc.py:704-708: log(x1 / x2), x clamped to [0, 1], x1 = max(x, eps), x2 = max(1 - x, eps).  `MLP.refine` fuses it into the box
    update; this form is for callers outside the decoder."""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def _host_sizes(spatial_shapes):
    """[(H, W)] on the host; a GPU tensor is read back, as the reference's loop over it does."""
    if torch.is_tensor(spatial_shapes):
        spatial_shapes = spatial_shapes.tolist()
    return [(int(h), int(w)) for h, w in spatial_shapes]


def gen_encoder_output_proposals(memory, memory_padding_mask, spatial_shapes, learnedwh=None, want_keep=False):
    """:56-116 in one launch (`ops.gdino_proposals`): memory [bs, sum(HW), C], memory_padding_mask bool [bs, sum(HW)] (True = padding),
    spatial_shapes [levels, 2] -> (output_memory: memory with the padded and the invalid rows zeroed, in memory's dtype; output_proposals fp32
    [bs, sum(HW), 4], un-sigmoided, +inf on those rows).  `want_keep` (ours) appends the uint8 [bs, sum(HW)] flag of the kept rows."""
    if learnedwh is not None:
        raise NotImplementedError("gen_encoder_output_proposals: learnedwh is not built on the HIP path (no GroundingDINO config sets it)")
    proposals, keep = ops.gdino_proposals(memory_padding_mask, _host_sizes(spatial_shapes))
    output_memory = memory.masked_fill((keep == 0)[..., None], 0.0)                # :110-111
    return (output_memory, proposals, keep) if want_keep else (output_memory, proposals)


def gen_sineembed_for_position(pos_tensor):
    """:204-230 for 4-d boxes (`ops.gdino_query_sine` at valid ratios of 1): pos_tensor fp32 [n_query, bs, 4] (x, y, w, h) -> [n_query, bs, 512]
    in (y, x, w, h) order.  The kernel stores the embedding as bf16 (it feeds a bf16 GEMM); it is returned widened to fp32."""
    if pos_tensor.size(-1) != 4:
        if pos_tensor.size(-1) == 2:
            raise NotImplementedError("gen_sineembed_for_position: 2-d points are not built on the HIP path (GroundingDINO's query_dim is 4)")
        raise ValueError("Unknown pos_tensor shape(-1):{}".format(pos_tensor.size(-1)))
    nq, bs, _ = pos_tensor.shape
    ones = torch.ones(nq, 1, 2, dtype=torch.float32, device=pos_tensor.device)
    _, emb = ops.gdino_query_sine(pos_tensor.detach().float().contiguous(), ones)
    return emb.view(nq, bs, 512).float()


class MLP(nn.Module):
    """:171-185, "very simple multi-layer perceptron".  Every layer runs in fp32 (`ops.linear_f32`): the MLPs of this model produce box coordinates,
    which feed sampling locations — the decision ms_deform_attn.py made for its projections.  `refine` is the box update of the decoder and the
    heads with the last layer fused into it."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def hidden(self, x):
        """The input of the last layer, fp32 [..., hidden_dim]."""
        x = x.detach().float()
        for layer in list(self.layers)[:-1]:
            x = F.relu(ops.linear_f32(x, layer.weight, layer.bias))
        return x

    def forward(self, x):
        last = self.layers[-1]
        return ops.linear_f32(self.hidden(x), last.weight, last.bias)

    def refine(self, x, reference, ref_is_logit=False, want_unsigmoid=False):
        """sigmoid(self(x) + inverse_sigmoid(reference)) (transformer.py:721-724, groundingdino.py:322-324) with the last layer, the inverse
        sigmoid and the sigmoid in one launch (`ops.gdino_box_refine`): x [..., input_dim], reference fp32 [..., 4] -> boxes fp32 [..., 4].
        ref_is_logit: reference is un-sigmoided already, +inf included (transformer.py:296-306).  want_unsigmoid also returns the sum."""
        last = self.layers[-1]
        if last.out_features != 4 or last.in_features != 256:
            raise ValueError(f"MLP.refine: the fused box update is built for a last layer of 256 -> 4, this one is {last.in_features} -> {last.out_features}")
        h = self.hidden(x)
        lead = h.shape[:-1]
        out = ops.gdino_box_refine(h.reshape(-1, 256), last.weight.detach(), last.bias.detach(), reference.detach().float().reshape(-1, 4).contiguous(),
                                   ref_is_logit=ref_is_logit, want_unsigmoid=want_unsigmoid)
        if want_unsigmoid:
            return out[0].view(*lead, 4), out[1].view(*lead, 4)
        return out.view(*lead, 4)


class ContrastiveEmbed(nn.Module):
    """:233-268: x [bs, n, C] against text_dict["encoded_text"] [bs, T, C] -> fp32 [bs, n, max_text_len], -inf at the tokens text_dict[
    "text_token_mask"] (True = used) leaves out and at columns T .. max_text_len-1.  Both operands are bf16 MFMA operands (`ops.contrastive`),
    the sums fp32.  `rowmax` (ours) is transformer.py:295, `forward(...).max(-1)[0]`, without the logits being stored."""

    def __init__(self, max_text_len=256):
        super().__init__()
        self.max_text_len = max_text_len

    def _operands(self, x, text_dict):
        assert isinstance(text_dict, dict)
        if x.dim() != 3:
            raise ValueError(f"ContrastiveEmbed: x must be [bs, n, C], got {tuple(x.shape)}")
        y = text_dict["encoded_text"]
        as_bf16 = lambda t: t.detach() if t.dtype == torch.bfloat16 else t.detach().to(torch.bfloat16)
        xb = as_bf16(x)
        if xb.stride(2) != 1 or (xb.shape[0] > 1 and xb.stride(0) != xb.shape[1] * xb.stride(1)):
            xb = xb.contiguous()
        return xb, as_bf16(y).contiguous(), text_dict["text_token_mask"]

    def forward(self, x, text_dict):
        xb, yb, mask = self._operands(x, text_dict)
        return ops.contrastive(xb, yb, mask, max_text_len=self.max_text_len)[0]

    def rowmax(self, x, text_dict):
        xb, yb, mask = self._operands(x, text_dict)
        return ops.contrastive(xb, yb, mask, max_text_len=self.max_text_len, want_logits=False, want_rowmax=True)[1]
