"""csrc/masactrl.hip on the GPU against the float64 statements of tests/masactrl_ref.py, on the same bf16 operands; then the editors on a small UNet.

Every kernel output sits between sentinel guards (tools/route_check.py's `Guarded`, or the byte / int32 twin below), is launched twice and must
repeat bit for bit, and every element is compared.  Each figure is printed before it is asserted.

Mutual attention: the bound of tools/route_check.py for the general attention kernel, whose arithmetic ae_attn_mutual_bf16 shares (fp32 logits from
bf16 MFMAs, fp32 softmax statistics, bf16 probabilities into the PV product, fp32 accumulation, one bf16 rounding of the output):
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j|      (`attn_out_bound`, `bound_check`).
A query of an empty class must give the mean of V under the same bound (its probabilities are the exact bf16 value 1, its denominator an fp32 count).

Token map, derivation of the bound from the kernel's arithmetic (token_map_kernel): a logit is an fp32 fma chain over D <= 160 bf16 products
(exact products, one rounding per step: |d s| <= D 2^-24 sum_d |q_d| |k_d| <= 2^-16 sum_d |q_d| |k_d|, the constant a of route_check.py), then
t = s c2 and t - m (two roundings, 2^-23 |t| together), then v_exp_f32 (1 ulp).  With E = (2^-16 + 2^-22) max_{h,j} scale sum_d |q_d| |k_jd| the
per-logit error in natural units, every probability moves by at most a factor e^{+-2E}, so the set's probability P_set by at most
2 E P_set (1 + O(E)).  The two wave sums add 128 non-negative fp32 terms in a 6-level tree plus the pair sum (<= 8 roundings: 2^-21 relative), the
division, the 1 / H scaling and the head sum add a few 2^-24 each.  Hence per launch
    |got - ref| <= (2.5 E + 2^-20) ref + 1e-12,
and an empty set is exactly 0 (its numerator is a sum of zeros).  With accumulate the bounds of the launches add, plus 2^-24 of the running sum
per addition (inside the 2^-20 term).

Classes: equal to the float64 classes everywhere except pixels whose float64 normalised value lies within masactrl_ref.CLS_BOUND of the threshold
(derived there); tests/test_masactrl_cpu.py shows the cases hold no such pixel except the one that meets the threshold exactly, where the arithmetic
is exact in both precisions — so these cases ask for equality outright, and the counts are the sums of the classes."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import masactrl_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from anyedit_amd import ops as o
    return o


@pytest.fixture(scope="module")
def RC():
    import route_check
    return route_check


class GuardedInts:
    """uint8 / int32 twin of route_check.Guarded: `shape` inside a flat allocation with sentinel-filled guards on both sides"""

    def __init__(self, shape, dtype, guard=4096):
        n = 1
        for s in shape:
            n *= s
        self.sent = 0xA5 if dtype == torch.uint8 else 0x5A5A5A5A
        self.buf = torch.full((guard + n + guard,), self.sent, dtype=dtype, device=DEV)
        self.view = self.buf[guard:guard + n].view(shape)
        self.g, self.n = guard, n

    def guards_intact(self):
        return bool((self.buf[:self.g] == self.sent).all()) and bool((self.buf[self.g + self.n:] == self.sent).all())


# ------------------------------------------------------------------------------------------------------------------ mutual attention
def _packed_operands(B, H, N, D, seed, pad=16):
    """q | k | v in place in a padded packed projection [B N, 3 inner + pad] (the pad columns hold NaN: they are never read)"""
    gen = torch.Generator().manual_seed(seed)
    inner = H * D
    ld = 3 * inner + pad
    buf = torch.randn(B * N, ld, generator=gen).to(BF)
    buf[:, 3 * inner:] = float("nan")
    st = (N * ld, D, ld)
    views = [buf.as_strided((B, H, N, D), st + (1,), i * inner).to(F64) for i in range(3)]
    return buf, st, views


def _run_mutual(ops, RC, B, H, N, D, src, qcls=None, kcls=None, kcnt=None, seed=0):
    buf, st, (Q, K, V) = _packed_operands(B, H, N, D, seed)
    inner = H * D
    dev = buf.to(DEV)
    dq, dk, dv = dev, dev[:, inner:], dev[:, 2 * inner:]
    dqc = None if qcls is None else qcls.to(DEV)
    dkc = None if kcls is None else kcls.to(DEV)
    if qcls is not None and kcnt is None:
        kcnt = torch.stack([(kcls == 0).sum(1), (kcls == 1).sum(1)], 1).to(torch.int32)
    dcnt = None if kcnt is None else kcnt.to(DEV)
    bits = []
    for _ in range(2):
        o = RC.Guarded(1, B * N * inner, BF, guard=4096)
        ops.attention_mutual(dq, dk, dv, B, H, N, D, D ** -0.5, st, st, st, src, qcls=dqc, kcls=dkc, kcnt=dcnt, out=o.view.reshape(B, N, inner))
        torch.cuda.synchronize()
        assert o.guards_intact(), "guard elements around the output were written"
        bits.append(o.bits())
    assert torch.equal(bits[0], bits[1]), "a second call is not bit-identical"
    assert torch.equal(dev.cpu().view(torch.int16), buf.view(torch.int16)), "the operands were modified"
    got = bits[0].view(BF).reshape(B, N, H, D).permute(0, 2, 1, 3).float()
    r, sv = R.mutual_ref(Q, K, V, D ** -0.5, src, qcls, kcls)
    ratio = RC.bound_check(got.reshape(-1, D), r.reshape(-1, D), RC.attn_out_bound(r, sv).reshape(-1, D), f"mutual B={B} N={N} D={D}")
    print(f"mutual B={B} H={H} N={N} D={D} src={tuple(src)} cls={qcls is not None}: worst err/bound {ratio:.3f}")
    return got, r


REMAP_N = (1, 25, 36, 81, 256, 1024)


@pytest.mark.parametrize("D", (40, 64, 80, 160))
@pytest.mark.parametrize("N", REMAP_N)
def test_mutual_remap(ops, RC, D, N):
    """the remap alone, B in {2, 4, 6}: the halves' sources ((b // n) n), and an arbitrary map"""
    i = REMAP_N.index(N) + (40, 64, 80, 160).index(D)
    B = (2, 4, 6)[i % 3]
    n = B // 2
    src = [(b // n) * n for b in range(B)]
    if i % 2:
        gen = torch.Generator().manual_seed(100 + i)
        src = [int(s) for s in torch.randint(0, B, (B,), generator=gen)]
    _run_mutual(ops, RC, B, 2, N, D, src, seed=10 * D + N)


def _class_pattern(kind, N, gen):
    """(qcls [4, N], kcls [4, N]) of the [u_s, u_t, c_s, c_t] batch: source rows ask for any key, target rows for the class of a seeded mask"""
    qcls = torch.full((4, N), R.CLS_ANY, dtype=torch.uint8)
    qt = torch.randint(0, 2, (2, N), generator=gen).to(torch.uint8)        # classes mixed within every query tile
    qt[torch.rand(2, N, generator=gen) < 0.1] = R.CLS_ANY                  # and some target queries that take every key
    if kind == "mixed":
        kc = torch.randint(0, 2, (N,), generator=gen)
    elif kind in ("edge32", "edge64"):
        e = 32 if kind == "edge32" else 64
        kc = (torch.arange(N) >= e).long()                                 # the class changes exactly at keys e-1 | e
    elif kind == "one":
        kc = torch.zeros(N, dtype=torch.long)
        kc[int(torch.randint(0, N, (1,), generator=gen))] = 1              # a class with one key
    elif kind == "any":
        kc = torch.randint(0, 2, (N,), generator=gen)
        qt[:] = R.CLS_ANY
    else:
        raise KeyError(kind)
    qcls[1], qcls[3] = qt[0], qt[1]
    kcls = kc.to(torch.uint8)[None].repeat(4, 1)
    kcls[2] = 1 - kcls[2] if kind != "one" else kcls[2].roll(3)            # the conditional half's source has its own classes
    return qcls, kcls.contiguous()


CLASS_CASES = [("mixed", 81), ("mixed", 1024), ("edge32", 36), ("edge32", 256), ("edge64", 81), ("edge64", 256), ("one", 25), ("one", 1024),
               ("any", 1), ("any", 81)]


@pytest.mark.parametrize("D", (40, 64, 80, 160))
@pytest.mark.parametrize("kind,N", CLASS_CASES, ids=[f"{k}-{n}" for k, n in CLASS_CASES])
def test_mutual_classes(ops, RC, D, kind, N):
    gen = torch.Generator().manual_seed(7 * N + D)
    qcls, kcls = _class_pattern(kind, N, gen)
    if kind in ("edge32", "edge64"):
        e = 32 if kind == "edge32" else 64
        assert int(kcls[0, e - 1]) != int(kcls[0, e])
    _run_mutual(ops, RC, 4, 2, N, D, (0, 0, 2, 2), qcls, kcls, seed=3 * N + D)


@pytest.mark.parametrize("D", (40, 64, 80, 160))
@pytest.mark.parametrize("S", (6, 16))
def test_mutual_empty_class_is_the_mean_of_v(ops, RC, D, S):
    """the unconditional half's source has no foreground key (classes and counts written by ae_masactrl_classes from a constant map), the
    conditional half's has no background key (a map that is >= thres everywhere but at its minimum ... which is one key: a one-key class too)"""
    N = S * S
    gen = torch.Generator().manual_seed(50 + S + D)
    maps = torch.rand(2, N, generator=gen) + 1.0
    maps[0] = 0.5                                               # constant: all-zero classes, counts (N, 0)
    cls, counts = GuardedInts((4, N), torch.uint8), GuardedInts((4, 2), torch.int32)
    ops.masactrl_classes(maps.to(DEV), S, S, 1e-6, [(0, 0), (1, 2)], cls.view, counts.view)
    torch.cuda.synchronize()
    assert cls.guards_intact() and counts.guards_intact()
    kcls, kcnt = cls.view.cpu(), counts.view.cpu()
    assert kcnt[0].tolist() == [N, 0] and kcnt[2].tolist() == [1, N - 1]
    kcls[1], kcls[3] = 0, 0                                     # rows the launch did not write (never read: src is 0 / 2)
    kcnt[1], kcnt[3] = 0, 0
    qcls = torch.full((4, N), R.CLS_ANY, dtype=torch.uint8)
    qcls[1] = torch.randint(0, 2, (N,), generator=gen).to(torch.uint8)
    qcls[3] = torch.randint(0, 2, (N,), generator=gen).to(torch.uint8)
    got, r = _run_mutual(ops, RC, 4, 2, N, D, (0, 0, 2, 2), qcls, kcls, kcnt=kcnt, seed=S + D)
    fg = qcls[1] == 1
    assert int(fg.sum()) > 0
    # the statement's rows ARE the mean of V (checked here so that the bound above was a bound on the mean)
    buf, st, (Q, K, V) = _packed_operands(4, 2, N, D, S + D)
    assert float((r[1][:, fg] - V[0].mean(1)[:, None, :]).abs().max()) < 1e-12


@pytest.mark.parametrize("N", (1, 65, 300))
def test_mutual_identity_equals_general_attention_bitwise(ops, N):
    """attn_mutual_kernel is the twin of attention.hip's attn_kernel (same tile constants, csrc/attn_tile.hpp; its own copy of the body): with the
    identity remap and no classes the mutual launch and ops.attention (head dim 64 reaches attn_kernel<64, 2, 4, true, 0, false> with no knob set) run the same arithmetic in the
    same order on the same packed operands, so their outputs are equal bit for bit (N: one row, a one-key tail tile, a ragged last query block)."""
    B, H, D = 2, 2, 64
    buf, st, _ = _packed_operands(B, H, N, D, 64 + N)
    inner = H * D
    dev = buf.to(DEV)
    got = ops.attention_mutual(dev, dev[:, inner:], dev[:, 2 * inner:], B, H, N, D, D ** -0.5, st, st, st, tuple(range(B)))
    want = ops.attention(dev, dev[:, inner:], dev[:, 2 * inner:], B, H, N, N, D, D ** -0.5, st, st, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    diff = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"mutual (identity, no classes) vs general attention, D={D} N={N}: {diff} differing elements of {got.numel()}")
    assert torch.equal(got, want)


_TWIN_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_hip_masactrl as TM
from anyedit_amd import ops
for N in (1, 65, 300):
    buf, st, _ = TM._packed_operands(2, 2, N, 40, 40 + N)
    dev = buf.to("cuda")
    got = ops.attention_mutual(dev, dev[:, 80:], dev[:, 160:], 2, 2, N, 40, 40 ** -0.5, st, st, st, (0, 1))
    want = ops.attention(dev, dev[:, 80:], dev[:, 160:], 2, 2, N, N, 40, 40 ** -0.5, st, st, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all()), N
    assert torch.equal(got, want), "N=%d: %d differing elements" % (N, int((got.view(torch.int16) != want.view(torch.int16)).sum()))
print("twins equal")
"""


def test_mutual_identity_equals_general_attention_bitwise_at_head_dim_40():
    """The same equality at head dim 40, which has the K = 16 tail operand and the ones row.  Head dim 40 reaches attn_kernel<40, 2, 4, true, 0, false> only
    with AE_ATTN_FAST=0, which attention.hip reads once per process: one child process under it runs N in {1, 65, 300}."""
    import subprocess
    env = dict(os.environ, AE_ATTN_FAST="0")
    r = subprocess.run([sys.executable, "-c", _TWIN_CHILD.format(tests=HERE, root=ROOT)], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "twins equal" in r.stdout


def test_mutual_refuses_other_head_dims(ops):
    from anyedit_amd._lib import lib, AnyEditHipError, check
    import ctypes
    x = torch.zeros(2 * 8, 3 * 32 + 16, dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="head dims"):
        ops.attention_mutual(x, x[:, 32:], x[:, 64:], 2, 1, 8, 32, 1.0, (8 * 112, 32, 112), (8 * 112, 32, 112), (8 * 112, 32, 112), (0, 0))
    out = torch.zeros(2, 8, 32, dtype=BF, device=DEV)
    arr = (ctypes.c_int * 2)(0, 0)
    rc = lib.ae_attn_mutual_bf16(x.data_ptr(), x[:, 32:].data_ptr(), x[:, 64:].data_ptr(), out.data_ptr(), 2, 1, 8, 32, 8 * 112, 32, 112, 8 * 112, 32, 112,
                                 8 * 112, 32, 112, 8 * 32, 32, 32, 1.0, arr, None, None, None, None)
    assert rc == -3                                             # AE_ERR_UNSUPPORTED
    with pytest.raises(AnyEditHipError, match="unsupported head_dim 32"):
        check(rc, "ae_attn_mutual_bf16")


# ------------------------------------------------------------------------------------------------------------------ token map
def _token_operands(B, H, N, Nk, D, seed):
    gen = torch.Generator().manual_seed(seed)
    inner = H * D
    ldq = inner + 8
    q = torch.randn(B * N, ldq, generator=gen).to(BF)
    q[:, inner:] = float("nan")
    kv = torch.randn(B * Nk, 2 * inner, generator=gen).to(BF)
    qs, ks = (N * ldq, D, ldq), (Nk * 2 * inner, D, 2 * inner)
    Q = q.as_strided((B, H, N, D), qs + (1,), 0).to(F64)
    K = kv.as_strided((B, H, Nk, D), ks + (1,), 0).to(F64)
    return q, kv, qs, ks, Q, K


def _token_sets(Nk, gen):
    """empty, one token (the last), all tokens, a seeded subset"""
    sub = [j for j in range(Nk) if float(torch.rand(1, generator=gen)) < 0.4]
    return [[], [Nk - 1], list(range(Nk)), sub]


def _token_bound(ref, qk_abs):
    E = (2.0 ** -16 + 2.0 ** -22) * qk_abs
    return (2.5 * E + 2.0 ** -20) * ref + 1e-12


@pytest.mark.parametrize("Nk", (1, 8, 77, 128))
@pytest.mark.parametrize("N", (1, 33, 256))
def test_token_map(ops, RC, N, Nk):
    i = (1, 33, 256).index(N) + (1, 8, 77, 128).index(Nk)
    H, D = ((2, 160), (5, 40), (3, 64))[i % 3]
    B = 4
    gen = torch.Generator().manual_seed(900 + 10 * N + Nk)
    q, kv, qs, ks, Q, K = _token_operands(B, H, N, Nk, D, 1000 + N + Nk)
    sets = _token_sets(Nk, gen)
    scale = D ** -0.5
    ref, qk_abs = R.token_map_ref(Q, K, scale, sets)
    dq, dkv = q.to(DEV), kv.to(DEV)
    bits = []
    for _ in range(2):
        o = RC.Guarded(1, B * N, torch.float32, guard=1024)
        ops.attention_token_map(dq, dkv, B, H, N, Nk, D, scale, qs, ks, sets, out=o.view.reshape(B, N))
        torch.cuda.synchronize()
        assert o.guards_intact()
        bits.append(o.bits())
    assert torch.equal(bits[0], bits[1]), "a second call is not bit-identical"
    got = bits[0].view(torch.float32).reshape(B, N)
    assert bool((got[0] == 0).all()), "an empty token set must give exactly 0"
    ratio = RC.bound_check(got, ref, _token_bound(ref, qk_abs), f"token map N={N} Nk={Nk} H={H} D={D}")
    print(f"token map N={N} Nk={Nk} H={H} D={D}: worst err/bound {ratio:.3f}; all-token row in [{float(got[2].min()):.7f}, {float(got[2].max()):.7f}]")


def test_token_map_accumulates_over_three_calls(ops, RC):
    B, H, N, Nk, D = 4, 2, 33, 77, 160
    total_ref = torch.zeros(B, N, dtype=F64)
    total_bnd = torch.zeros(B, N, dtype=F64)
    o = RC.Guarded(1, B * N, torch.float32, guard=1024)
    out = o.view.reshape(B, N)
    for c in range(3):
        gen = torch.Generator().manual_seed(40 + c)
        q, kv, qs, ks, Q, K = _token_operands(B, H, N, Nk, D, 70 + c)
        sets = _token_sets(Nk, gen)
        ref, qk_abs = R.token_map_ref(Q, K, D ** -0.5, sets)
        total_ref += ref
        total_bnd += _token_bound(ref, qk_abs)
        ops.attention_token_map(q.to(DEV), kv.to(DEV), B, H, N, Nk, D, D ** -0.5, qs, ks, sets, out=out, accumulate=c > 0)
    torch.cuda.synchronize()
    assert o.guards_intact()
    ratio = RC.bound_check(out.cpu(), total_ref, total_bnd + 2.0 ** -20 * total_ref, "token map, three accumulated calls")
    print(f"token map accumulate: worst err/bound {ratio:.3f}")
    with pytest.raises(ValueError, match="accumulate needs"):
        ops.attention_token_map(q.to(DEV), kv.to(DEV), B, H, N, Nk, D, D ** -0.5, qs, ks, sets, accumulate=True)
    with pytest.raises(ValueError, match="Nk <= 128"):
        ops.attention_token_map(q.to(DEV), kv.to(DEV), B, H, N, 129, D, D ** -0.5, qs, ks, sets)


# ------------------------------------------------------------------------------------------------------------------ classes
@pytest.mark.parametrize("case", R.CLASS_CASES, ids=[c[0] for c in R.CLASS_CASES])
def test_classes(ops, case):
    _, S, R_, thres, kind, seed = case
    maps = R.class_case_maps(S, kind, seed)
    pairs = [(0, 2), (1, 0), (2, 1), (1, 3)]
    bits = []
    for _ in range(2):
        cls, counts = GuardedInts((4, R_ * R_), torch.uint8), GuardedInts((4, 2), torch.int32)
        ops.masactrl_classes(maps.to(DEV), S, R_, thres, pairs, cls.view, counts.view)
        torch.cuda.synchronize()
        assert cls.guards_intact() and counts.guards_intact()
        bits.append((cls.view.cpu(), counts.view.cpu()))
    assert torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1])
    got, cnt = bits[0]
    for s, o in pairs:
        want, wcnt, norm = R.classes_ref(maps[s], S, R_, thres)
        near = (norm - thres).abs() <= R.CLS_BOUND
        if kind == "exact" and s == 1:
            near[:] = False                                    # exact arithmetic on both sides: the pixel on the threshold is class 1 here too
        assert int(near.sum()) <= 0.01 * R_ * R_
        diff = (got[o] != want) & ~near
        print(f"classes {case[0]} map {s} -> row {o}: ones {int(got[o].sum())} (float64 {int(want.sum())}), near the threshold {int(near.sum())}, differing {int(diff.sum())}")
        assert int(diff.sum()) == 0
        assert cnt[o].tolist() == [R_ * R_ - int(got[o].sum()), int(got[o].sum())]
        if kind == "constant" and s == 1:
            assert int(got[o].sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ module level
UNET64 = dict(image_size=32, in_channels=8, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=[1, 2], channel_mult=[1, 2],
              num_head_channels=64, use_spatial_transformer=True, transformer_depth=1, context_dim=16, legacy=False, use_checkpoint=False)


@pytest.fixture(scope="module")
def small_ldm():
    """the tiny UNet of util_models.py at head dim 64 (the kernels' smallest) on 32 x 32 latents: transformer blocks at 1024 and 256 tokens"""
    from util_models import G, unzero, randomize_norm_affine
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from anyedit_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    torch.manual_seed(51)
    g = G(51)
    unet = UNetModel(**UNET64)
    unzero(unet, g, std=0.05)
    randomize_norm_affine(unet, g)
    return LatentDiffusion(unet.eval(), conditioning_key="hybrid", timesteps=1000, linear_start=0.00085, linear_end=0.0120).to(DEV)


class _Composition:
    """Mix-in for the editor classes: the same decisions (counting, gating, classes) carried out by the operators the library had before
    ae_attn_mutual_bf16 — per masked call a source launch, two `key_mask` launches of the target rows on the source's keys and a blend."""

    def _plain(self, attn, B, N, qkv):
        from anyedit_amd import ops
        h, d = attn.heads, attn.dim_head
        inner = h * d
        s = (N * 3 * inner, d, 3 * inner)
        n = B // 2
        kv = qkv.reshape(B, N, 3 * inner)[[(b // n) * n for b in range(B)]].reshape(B * N, 3 * inner).contiguous()   # the sources' rows, copied
        return ops.attention(qkv, kv[:, inner:], kv[:, 2 * inner:], B, h, N, N, d, attn.scale, s, s, s)

    def _masked(self, attn, B, N, qkv, qcls, kcls, kcnt):
        from anyedit_amd import ops
        h, d = attn.heads, attn.dim_head
        inner = h * d
        s = (N * 3 * inner, d, 3 * inner)
        kv = qkv.reshape(B, N, 3 * inner)[[0, 0, 2, 2]].reshape(B * N, 3 * inner).contiguous()
        k, v = kv[:, inner:], kv[:, 2 * inner:]
        kcls = kcls[[0, 0, 2, 2]]                                                                             # key_mask goes by the query's sample
        o_all = ops.attention(qkv, k, v, B, h, N, N, d, attn.scale, s, s, s)                                  # source rows (and "any" queries)
        o_fg = ops.attention(qkv, k, v, B, h, N, N, d, attn.scale, s, s, s, key_mask=(kcls == 1).to(torch.uint8).contiguous())
        o_bg = ops.attention(qkv, k, v, B, h, N, N, d, attn.scale, s, s, s, key_mask=(kcls == 0).to(torch.uint8).contiguous())
        q = qcls[:, :, None]
        return torch.where(q == 1, o_fg, torch.where(q == 0, o_bg, o_all))


def _editors(kind, composition):
    import anyedit_amd.masactrl as M
    import anyedit_amd.masactrl.masactrl as MM
    kw = dict(start_step=1, start_layer=2, total_steps=2)
    base = {"plain": M.MutualSelfAttentionControl, "mask": M.MutualSelfAttentionControlMask, "auto": M.MutualSelfAttentionControlMaskAuto}[kind]
    if kind == "mask":
        yy, xx = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
        kw.update(mask_s=(((yy - 14) ** 2 + (xx - 12) ** 2) < 81).float(), mask_t=(((yy - 18) ** 2 + (xx - 20) ** 2) < 64).float())
    if kind == "auto":
        kw.update(thres=0.5, ref_token_idx=[1], cur_token_idx=[1, 2])
    if not composition:
        return base(**kw)

    class Comp(_Composition, base):
        pass

    ed = Comp(**kw)
    if kind != "plain":     # the masked calls go through `_mutual`: give the composition editor its own
        ed._use_composition = True
    return ed


def _inputs():
    gen = torch.Generator().manual_seed(5)
    x_1 = torch.randn(1, 4, 32, 32, generator=gen).to(DEV)
    img = torch.randn(2, 4, 32, 32, generator=gen).to(DEV)
    ctx, null = torch.randn(2, 8, 16, generator=gen).to(DEV), torch.randn(1, 8, 16, generator=gen).expand(2, -1, -1).contiguous().to(DEV)
    return x_1, img, ctx, null


def _sample(ldm, editor, record):
    """two DDIM steps with classifier-free guidance on a (source, target) pair: UNet batches of [u_s, u_t, c_s, c_t]"""
    import anyedit_amd.masactrl as M
    import anyedit_amd.masactrl.masactrl as MM
    from anyedit_amd.ldm.models.diffusion.ddim import DDIMSampler
    x_1, img, ctx, null = _inputs()
    x_T = x_1.expand(2, -1, -1, -1).contiguous()
    model = type("W", (), {})()
    model.model = ldm.model
    orig_mutual = MM._mutual
    if editor is not None:
        M.register_attention_editor_ldm(model, editor)
        assert editor.num_att_layers == 14
        inner_call = editor.forward

        def recording(attn, is_cross, B, N, core, **operands):
            o = inner_call(attn, is_cross, B, N, core, **operands)
            if not is_cross:
                record.append(o.float().cpu())
            return o
        editor.forward = recording
        if getattr(editor, "_use_composition", False):
            MM._mutual = lambda attn, B, N, qkv, src, qcls, kcls, kcnt: editor._masked(attn, B, N, qkv, qcls, kcls, kcnt)
    try:
        sampler = DDIMSampler(ldm)
        cond = {"c_concat": [img], "c_crossattn": [ctx]}
        uncond = {"c_concat": [img], "c_crossattn": [null]}
        samples, _ = sampler.sample(2, 2, (4, 32, 32), cond, eta=0.0, x_T=x_T, verbose=False, unconditional_guidance_scale=7.5,
                                    unconditional_conditioning=uncond)
    finally:
        MM._mutual = orig_mutual
        if editor is not None:
            assert M.unregister(model) == 14
    return samples.float().cpu()


@pytest.fixture(scope="module")
def never_registered(small_ldm):
    return _sample(small_ldm, None, [])


@pytest.mark.parametrize("kind", ("plain", "mask", "auto"))
def test_editors_on_the_unet(small_ldm, never_registered, kind):
    """Each editor registered on the UNet, two DDIM steps across the start step, against the same model with the editor's decisions carried out
    by the composition of the existing operators.  Attention outputs: relative L2 6e-3 / max-abs over max 3e-2 (the forward output's tolerance
    of test_hip_attention_training.py); latents: tests/test_hip_unet.py's `close` (relative L2 2e-2, 38 dB).  With the editor unregistered the
    latents are bit-identical to those of a model that never had one."""
    from conftest import rel_l2, psnr
    rec_a, rec_b = [], []
    ed = _editors(kind, False)
    got = _sample(small_ldm, ed, rec_a)
    want = _sample(small_ldm, _editors(kind, True), rec_b)
    assert ed.cur_step == 2 and ed.cur_att_layer == 0
    assert ed.controlled == [(1, 2 * b) for b in range(2, 7)], ed.controlled
    assert len(rec_a) == len(rec_b) == 14
    worst = (0.0, 0.0)
    for i, (a, b) in enumerate(zip(rec_a, rec_b)):
        e, m = rel_l2(a, b), float((a - b).abs().max() / b.abs().max())
        worst = (max(worst[0], e), max(worst[1], m))
        if i < 7 + 2:       # step 0 and the blocks below the start layer: the same launches on the same operands
            assert torch.equal(a, b), f"{kind}: uncontrolled self-attention {i} differs"
    print(f"{kind}: attention outputs worst rel_l2 {worst[0]:.3e} (<= 6e-3), max_abs/max {worst[1]:.3e} (<= 3e-2)")
    e, p = rel_l2(got, want), psnr(got, want)
    print(f"{kind}: latents rel_l2 {e:.3e} (<= 2e-2), psnr {p:.1f} dB (>= 38); against the unedited pair rel_l2 {rel_l2(got, never_registered):.3e}")
    assert worst[0] <= 6e-3 and worst[1] <= 3e-2
    assert e <= 2e-2 and p >= 38.0
    assert not torch.equal(got[1], never_registered[1]), "the editor changed nothing on the target"
    again = _sample(small_ldm, None, [])
    assert torch.equal(again, never_registered), "after unregister the latents must be bit-identical to a model that never had an editor"


def test_consistent_synthesis_is_the_registered_sampler_run(small_ldm, monkeypatch):
    """anyedit_amd.tools.masactrl_synthesis.consistent_synthesis: one start code expanded over the prompts, the editor registered for the run and
    removed afterwards, DDIM with classifier-free guidance — bit-identical to the same run set up by hand (the text encoder and the decoder are
    stubbed: they are not what this function adds)."""
    from anyedit_amd.ldm.models.diffusion.ddim import DDIMSampler
    from anyedit_amd.ldm.modules.attention import CrossAttention
    from anyedit_amd.tools.masactrl_synthesis import consistent_synthesis
    x_1, img, ctx, null = _inputs()
    monkeypatch.setattr(small_ldm, "get_learned_conditioning", lambda p: {"c_concat": [img], "c_crossattn": [null if p[0] == "" else ctx]}, raising=False)
    monkeypatch.setattr(small_ldm, "decode_first_stage", lambda z: z, raising=False)
    out = consistent_synthesis(small_ldm, DDIMSampler(small_ldm), ["a person standing", "a person jumping"], start_code=x_1, step=1, layer=2,
                               guidance_scale=7.5, steps=2)
    want = _sample(small_ldm, _editors("plain", False), [])
    assert torch.equal(out.float().cpu(), want)
    assert not any("editor" in m.__dict__ for m in small_ldm.modules() if isinstance(m, CrossAttention))
    with pytest.raises(ValueError, match="start_code"):
        consistent_synthesis(small_ldm, DDIMSampler(small_ldm), ["a", "b"], start_code=x_1.expand(2, -1, -1, -1))
