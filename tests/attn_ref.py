"""Plain float64 restatement of one softmax-attention segment, forward and backward, by its explicit formulas — test infrastructure: the
CPU suite pins it to torch.autograd (tests/test_attn_ref.py), the GPU suite (tests/test_hip_attention_training.py) compares
ae_attn_fwd_bf16 / ae_attn_bwd_bf16 with it on the same bf16-rounded operands.

    S = scale Q K^T     P = softmax(S)     O = P V     L2 = log2 sum_j exp(S_j)              (forward; L2 is what the kernels store as lse)
    dV = g P^T dO       dP = dO V^T        delta = rowsum(P o dP)                            (delta: un-scaled — no g)
    dS = P o (dP - delta) scale            dQ = g dS K          dK = g dS^T Q
g = the optional per-batch output scale (the adapter gate: out = Attn(q, K, V) + g_b Attn(q, K2, V2)); d out / d g_b = sum_{h, q} delta.
"""
import torch

F64 = torch.float64
LOG2E = 1.4426950408889634


def view4(t, B, H, n, D, strides, offset=0):
    """(B, H, n, D) float64 copy of an operand addressed through (batch, head, row) element strides from `offset` of t's storage"""
    return t.as_strided((B, H, n, D), tuple(strides) + (1,), t.storage_offset() + offset).to(F64)


def segment(Q, K, V, scale, dO=None, gate=None, given_lse=None, given_delta=None):
    """Q [B, H, Nq, D], K / V [B, H, Nk, D], dO [B, H, Nq, D] (float64), gate [B] or None.  Returns a dict: out (un-gated P V), lse (L2),
    and with dO: delta, dq, dk, dv (gated), dgate [B].
    given_lse / given_delta [B, H, Nq]: the backward as a function of ITS inputs — ae_attn_bwd_bf16 does not normalise, it takes
    P = 2^(log2(e) S - L2) from the L2 it is handed (and delta = rowsum(dO o out) from the output it is handed): with these the
    backward formulas are evaluated at that L2 / delta instead of the exact ones (`out` and `lse` stay exact)."""
    Q, K, V = Q.to(F64), K.to(F64), V.to(F64)
    S = scale * (Q @ K.transpose(-1, -2))
    m = S.max(-1, keepdim=True).values
    E = torch.exp(S - m)
    den = E.sum(-1, keepdim=True)
    P = E / den
    res = dict(out=P @ V, lse=((m + torch.log(den)) * LOG2E).squeeze(-1))
    if dO is None:
        return res
    dO = dO.to(F64)
    g = torch.ones(Q.shape[0], dtype=F64) if gate is None else gate.to(F64)
    g4 = g[:, None, None, None]
    if given_lse is not None:
        P = torch.exp(S - given_lse.to(F64)[..., None] / LOG2E)
    dP = dO @ V.transpose(-1, -2)
    delta = (P * dP).sum(-1) if given_delta is None else given_delta.to(F64)
    dS = P * (dP - delta[..., None]) * scale
    res.update(delta=delta, dv=g4 * (P.transpose(-1, -2) @ dO), dq=g4 * (dS @ K), dk=g4 * (dS.transpose(-1, -2) @ Q), dgate=delta.sum((1, 2)))
    return res
