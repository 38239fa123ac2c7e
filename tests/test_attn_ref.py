"""tests/attn_ref.py (the float64 formulas the GPU attention tests compare with) against torch.autograd of softmax attention in float64."""
import pytest
import torch

import attn_ref as R

F64 = torch.float64


def _attn(q, k, v, scale):
    return torch.softmax(scale * (q @ k.transpose(-1, -2)), -1) @ v


def _close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)
    assert err <= 1e-10, f"{what}: {err:.3e}"


@pytest.mark.parametrize("mode", ["one_segment", "gated", "two_segments_with_gate"])
def test_formulas_agree_with_autograd(mode):
    B, H, Nq, Nk, Nk2, D = 2, 3, 19, 13, 5, 24
    g = torch.Generator().manual_seed(11)
    q, k, v, k2, v2 = (torch.randn(B, H, n, D, generator=g, dtype=F64).requires_grad_(True) for n in (Nq, Nk, Nk, Nk2, Nk2))
    dO = torch.randn(B, H, Nq, D, generator=g, dtype=F64)
    gate = torch.tensor([0.7, 1.3], dtype=F64, requires_grad=True)
    scale = D ** -0.5
    g4 = gate[:, None, None, None]
    first = _attn(q, k, v, scale)
    out = first if mode == "one_segment" else g4 * first if mode == "gated" else first + g4 * _attn(q, k2, v2, scale)
    out.backward(dO)
    with torch.no_grad():
        r1 = R.segment(q, k, v, scale, dO, gate=gate if mode == "gated" else None)
        _close(r1["out"], first, "out")
        _close(r1["lse"], torch.logsumexp(scale * (q @ k.transpose(-1, -2)), -1) * R.LOG2E, "lse")
        _close(r1["delta"], (dO * first).sum(-1), "delta = rowsum(dO o O), un-scaled")
        _close(r1["dk"], k.grad, "dK")
        _close(r1["dv"], v.grad, "dV")
        if mode == "two_segments_with_gate":
            r2 = R.segment(q, k2, v2, scale, dO, gate=gate)
            _close(r1["dq"] + r2["dq"], q.grad, "dQ (both segments)")
            _close(r2["dk"], k2.grad, "dK2")
            _close(r2["dv"], v2.grad, "dV2")
            _close(r2["dgate"], gate.grad, "gate gradient = sum of the second segment's delta")
        else:
            _close(r1["dq"], q.grad, "dQ")
            if mode == "gated":
                _close(r1["dgate"], gate.grad, "gate gradient = sum of delta")


def test_given_lse_and_delta_reproduce_the_exact_backward_and_shift_it_as_derived():
    """segment(given_lse=, given_delta=): at the exact values nothing changes; an lse that is off by e (natural units) scales every
    probability of the row by exp(-e): dV and the un-normalised delta scale with it row by row."""
    B, H, Nq, Nk, D = 2, 3, 7, 9, 16
    g = torch.Generator().manual_seed(3)
    q, k, v, dO = (torch.randn(B, H, n, D, generator=g, dtype=F64) for n in (Nq, Nk, Nk, Nq))
    exact = R.segment(q, k, v, 0.25, dO)
    same = R.segment(q, k, v, 0.25, dO, given_lse=exact["lse"], given_delta=exact["delta"])
    for name in ("delta", "dq", "dk", "dv"):
        _close(same[name], exact[name], name)
    e = 0.01 * torch.randn(B, H, Nq, generator=g, dtype=F64)
    off = R.segment(q, k, v, 0.25, dO, given_lse=exact["lse"] + e * R.LOG2E)
    _close(off["delta"], torch.exp(-e) * exact["delta"], "delta at a shifted lse")
    _close(off["lse"], exact["lse"], "the forward part stays exact")


def test_view4_follows_the_strides():
    B, H, N, D = 2, 3, 5, 8
    C = H * D
    rows = torch.arange(B * N * (3 * C + 8), dtype=torch.float32).reshape(B * N, 3 * C + 8)
    k = R.view4(rows, B, H, N, D, (N * (3 * C + 8), D, 3 * C + 8), offset=C)
    assert torch.equal(k, rows[:, C:2 * C].reshape(B, N, H, D).permute(0, 2, 1, 3).double())
