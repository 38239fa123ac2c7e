"""csrc/prompt2prompt.hip on the GPU against the float64 statements of tests/p2p_ref.py, on the same bf16 operands; then the controllers on a small UNet.

Every kernel output sits between sentinel guards (tools/route_check.py's `Guarded`), is launched twice and must repeat bit for bit, the operands
are verified unmodified, every element is compared, and each figure is printed before it is asserted.

Edited attention, the output bound (p2p_ref.p2p_out_bound, derived there from the kernel's arithmetic):
    |got - ref| <= 2^-8 |ref| + kappa 2^-8 sum_j w_j |v_j|,   w_j = |c_j| (P_base |M|)_j + |d_j| P_own,j.
kappa counts the bf16 roundings on the probability path.  ae_attn_p2p_bf16 forms P_base M in fp32 on the VALU and keeps P' in fp32 into an fp32 fma
chain over the keys: there is NO bf16 rounding on that path (the existing MFMA kernels have one, kappa = 1).  kappa 2^-8 is therefore replaced by
the relative error of the fp32 path, eps_prob + (2 Nk + 2) 2^-24 with eps_prob = 2 (D + 2) 2^-24 max scale sum_d |q_d| |k_d| + 2^-20: a few 1e-5 at
these operands, two orders below 2^-8.  The store bound (p2p_ref.p2p_store_bound) follows the token-map derivation of tests/test_hip_masactrl.py
with the same eps_prob, per (row, key) entry instead of per token set, plus one 2^-24 per head and per accumulating launch.  Entries whose w_j is
exactly 0 must be exactly 0 in the store.

Local blend: the mask must equal the float64 mask outside a band of p2p_ref.blend_band around the threshold; tests/test_p2p_cpu.py asserts that the
seeded cases put no pixel inside the band (except pixels whose arithmetic is exact in both precisions), so equality is asked for outright; the
blended latents are x[1] bit for bit where the mask is 1 and x[0] bit for bit where it is 0."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import p2p_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
GOLDEN = os.path.join(HERE, "golden", "p2p.npz")


@pytest.fixture(scope="module")
def ops():
    from anyedit_amd import ops as o
    return o


@pytest.fixture(scope="module")
def RC():
    import route_check
    return route_check


@pytest.fixture(scope="module")
def tables():
    return R.golden_tables(R.load_golden(GOLDEN))


class _Case:
    """operands of a kernel case on both sides, shared by the variants of one test"""

    def __init__(self, case):
        self.case = case
        self.D, self.Nk, self.N, self.H, self.B = case
        self.q, self.kv, self.qs, self.ks, self.Q, self.K, self.V = R.case_operands(case)
        self.dq, self.dkv = self.q.to(DEV), self.kv.to(DEV)
        self.inner = self.H * self.D
        self.scale = self.D ** -0.5
        self.qk = R.qk_abs(self.Q, self.K, self.scale)
        self.base = R.case_base(self.B)

    def launch(self, ops, RC, M, c, d, store_rows=None, accumulate=False, want_out=True, prefill=None, base=None):
        """two launches between guards; returns (out float [B, H, N, D] or None, store float32 [rows, N, Nk] or None)"""
        B, H, N, Nk, D = self.B, self.H, self.N, self.Nk, self.D
        dM, dc, dd = (None if t is None else t.to(DEV) for t in (M, c, d))
        bits, sbits = [], []
        for _ in range(2):
            o = RC.Guarded(1, B * N * self.inner, BF, guard=4096) if want_out else None
            st = None
            if store_rows is not None:
                rows = max(store_rows) + 1
                st = RC.Guarded(1, rows * N * Nk, torch.float32, guard=4096)
                if prefill is not None:
                    st.view.reshape(rows, N, Nk).copy_(prefill.to(DEV))
            ops.attention_p2p(self.dq, self.dkv, self.dkv[:, self.inner:], B, H, N, Nk, D, self.scale, self.qs, self.ks, self.ks,
                              self.base if base is None else base, M=dM, c=dc, d=dd,
                              store=None if st is None else st.view.reshape(rows, N, Nk), store_row=store_rows, accumulate=accumulate,
                              out=None if o is None else o.view.reshape(B, N, self.inner), want_out=want_out)
            torch.cuda.synchronize()
            if o is not None:
                assert o.guards_intact(), "guard elements around the output were written"
                bits.append(o.bits())
            if st is not None:
                assert st.guards_intact(), "guard elements around the store were written"
                sbits.append(st.bits())
        if bits:
            assert torch.equal(bits[0], bits[1]), "a second call is not bit-identical (output)"
        if sbits:
            assert torch.equal(sbits[0], sbits[1]), "a second call is not bit-identical (store)"
        assert torch.equal(self.dq.cpu().view(torch.int16), self.q.view(torch.int16)), "q was modified"
        assert torch.equal(self.dkv.cpu().view(torch.int16), self.kv.view(torch.int16)), "k / v were modified"
        out = bits[0].view(BF).reshape(B, N, H, D).permute(0, 2, 1, 3).float() if bits else None
        store = sbits[0].view(torch.float32).reshape(-1, N, Nk) if sbits else None
        return out, store

    def check_out(self, RC, got, M, c, d, what):
        ref, Pp, W = R.p2p_ref(self.Q, self.K, self.V, self.scale, self.base, M, c, d)
        bnd = R.p2p_out_bound(ref, W, self.V, self.D, self.Nk, self.qk)
        ratio = RC.bound_check(got.reshape(-1, self.D), ref.reshape(-1, self.D), bnd.reshape(-1, self.D), what)
        print(f"{what}: output worst err/bound {ratio:.3f}")
        return ref, Pp, W

    def check_store(self, RC, got, Pp, W, rows, what, launches=1, offset=None):
        """got [n, N, Nk]; sample b of the batch sits in row rows[b] (or -1)"""
        ref_all, bnd_all = Pp.sum(1), R.p2p_store_bound(W, self.Nk, self.D, self.qk, self.H, launches)
        for b, r in enumerate(rows):
            if r < 0:
                continue
            ref, bnd = ref_all[b] * launches, bnd_all[b] * launches
            if offset is not None:
                ref = ref + offset[r].to(F64)
                bnd = bnd + 2.0 ** -24 * offset[r].to(F64).abs()
            zero = W.sum(1)[b] == 0
            if offset is None:
                assert bool((got[r][zero] == 0).all()), f"{what}: an entry whose weights are exactly 0 is not exactly 0"
            ratio = RC.bound_check(got[r], ref, bnd, f"{what} store row {r}")
            print(f"{what}: store row {r} (sample {b}) worst err/bound {ratio:.3f}; exactly-zero entries {int(zero.sum())}")


CASES = R.p2p_cases()


@pytest.mark.parametrize("case", CASES, ids=[R.case_id(c) for c in CASES])
def test_attention_p2p(ops, RC, tables, case):
    """one case of the walk: a dense random edit with the store overwritten, c = 0, the store accumulated over two launches, the store alone
    (no output), the golden's tables at 77 keys, and the refusals"""
    cs = _Case(case)
    B, P, N, Nk = cs.B, cs.B // 2, cs.N, cs.Nk
    rows = [-1] * P + list(range(P))
    what = "p2p " + R.case_id(case)
    # dense M, mixed signs, some (c, d) pairs exactly zero; output and store in one launch
    M, c, d = R.case_edit(case, "dense")
    got, store = cs.launch(ops, RC, M, c, d, store_rows=rows)
    _, Pp, W = cs.check_out(RC, got, M, c, d, what + " dense")
    cs.check_store(RC, store, Pp, W, rows, what + " dense")
    unedited, _, _ = R.p2p_ref(cs.Q, cs.K, cs.V, cs.scale, list(range(B)))
    # the store alone: the same bits as the store of the launch that also wrote the output
    _, store_only = cs.launch(ops, RC, M, c, d, store_rows=rows, want_out=False)
    assert torch.equal(store_only, store), "the store-only launch differs from the store of the full launch"
    # accumulate onto a prefilled store, rows permuted
    gen = torch.Generator().manual_seed(11)
    rows2 = [-1] * P + list(reversed(range(P)))
    pre = torch.rand(P, N, Nk, generator=gen)
    _, acc = cs.launch(ops, RC, M, c, d, store_rows=rows2, accumulate=True, want_out=False, prefill=pre)
    cs.check_store(RC, acc, Pp, W, rows2, what + " accumulate", offset=pre)
    # c = 0, d = 1: the unedited result under the bound
    M0, c0, d0 = R.case_edit(case, "czero")
    got0, _ = cs.launch(ops, RC, M0, c0, d0)
    ref0, _, W0 = cs.check_out(RC, got0, M0, c0, d0, what + " c=0")
    ratio = RC.bound_check(got0.reshape(-1, cs.D), unedited.reshape(-1, cs.D), R.p2p_out_bound(unedited, W0, cs.V, cs.D, Nk, cs.qk).reshape(-1, cs.D),
                           what + " c=0 against the unedited statement")
    print(f"{what} c=0 vs unedited: worst err/bound {ratio:.3f}")
    if Nk == 77:
        for variant in ("replace", "refine", "reweight"):
            Mt, ct, dt = R.case_edit(case, variant, tables)
            gt, st = cs.launch(ops, RC, Mt, ct, dt, store_rows=rows)
            _, Ppt, Wt = cs.check_out(RC, gt, Mt, ct, dt, f"{what} {variant}")
            cs.check_store(RC, st, Ppt, Wt, rows, f"{what} {variant}")
    # an edited sample whose base is itself edited is refused on the host, before any launch
    bad = list(cs.base)
    bad[B - 1] = B - 2
    if B > 4:
        with pytest.raises(ValueError, match="must be unedited"):
            cs.launch(ops, RC, M, c, d, base=bad)


def test_attention_p2p_refusals(ops):
    from anyedit_amd import _lib
    import ctypes
    B, H, N, Nk, D = 4, 2, 17, 77, 64
    q = torch.zeros(B * N, H * D, dtype=BF, device=DEV)
    kv = torch.zeros(B * Nk, 2 * H * D, dtype=BF, device=DEV)
    qs, ks = (N * H * D, D, H * D), (Nk * 2 * H * D, D, 2 * H * D)
    c = torch.zeros(B, Nk, device=DEV)
    with pytest.raises(ValueError, match="head dims"):
        ops.attention_p2p(q, kv, kv, B, H, N, Nk, 48, 0.1, qs, ks, ks, [0, 1, 2, 2], c=c, d=c)
    with pytest.raises(ValueError, match="Nk <= 128"):
        ops.attention_p2p(q, kv, kv, B, H, N, 129, D, 0.1, qs, ks, ks, [0, 1, 2, 2], c=c, d=c)
    with pytest.raises(ValueError, match="needs c and d"):
        ops.attention_p2p(q, kv, kv[:, H * D:], B, H, N, Nk, D, 0.1, qs, ks, ks, [0, 1, 2, 2])
    with pytest.raises(ValueError, match="needs a store"):
        ops.attention_p2p(q, kv, None, B, H, N, Nk, D, 0.1, qs, ks, ks, [0, 1, 2, 3], want_out=False)
    # the library itself refuses what ops refuses: a base that is edited, an unsupported head dim (before any launch)
    o = torch.empty(B, N, H * D, dtype=BF, device=DEV)
    arr = (ctypes.c_int * B)(0, 1, 3, 2)
    rc = _lib.lib.ae_attn_p2p_bf16(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), o.data_ptr(), B, H, N, Nk, D, *qs, *ks, *ks, N * H * D, D, H * D, 0.1, arr,
                                   None, c.data_ptr(), c.data_ptr(), None, None, 0, 0, None)
    assert rc != 0 and b"itself an edited sample" in _lib.lib.ae_last_error()
    arr = (ctypes.c_int * B)(0, 1, 2, 2)
    rc = _lib.lib.ae_attn_p2p_bf16(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), o.data_ptr(), B, H, N, Nk, 48, *qs, *ks, *ks, N * H * D, D, H * D, 0.1, arr,
                                   None, c.data_ptr(), c.data_ptr(), None, None, 0, 0, None)
    assert rc == -3 and b"head_dim 48" in _lib.lib.ae_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ local blend
@pytest.mark.parametrize("case", R.BLEND_CASES, ids=[c[0] for c in R.BLEND_CASES])
def test_local_blend(ops, RC, case):
    _, S, (h, w), L, kind, _ = case
    maps, sets, thr, x = R.blend_case(case)
    want, mask, norm = R.blend_ref(maps, sets, S, thr, x)
    dmaps, dx = [m.to(DEV) for m in maps], x.to(DEV)
    bits = []
    for _ in range(2):
        o = RC.Guarded(1, x.numel(), torch.float32, guard=4096)
        ops.p2p_local_blend(dmaps, S, R.BLEND_NK, sets, thr, dx, out=o.view.reshape(x.shape))
        torch.cuda.synchronize()
        assert o.guards_intact()
        bits.append(o.bits())
    assert torch.equal(bits[0], bits[1]), "a second call is not bit-identical"
    assert torch.equal(dx.cpu(), x) and all(torch.equal(a.cpu(), b) for a, b in zip(dmaps, maps)), "the inputs were modified"
    got = bits[0].view(torch.float32).reshape(x.shape)
    xi = x.view(torch.int32)
    gi = got.view(torch.int32)
    is1 = (gi[1] == xi[1]).all(0)
    is0 = (gi[1] == xi[0]).all(0)
    print(f"blend {case[0]}: mask ones {int(mask.sum())} of {h * w} (float64), pixels equal to x[1] {int(is1.sum())}, to x[0] {int(is0.sum())}")
    assert torch.equal(gi[0], xi[0]), "out[0] must be x[0] bit for bit"
    assert bool(is1[mask].all()), "where the mask is 1 the blended latents must equal x[1] bit for bit"
    assert bool(is0[~mask].all()), "where the mask is 0 the blended latents must equal x[0] bit for bit"
    if kind in ("random",):
        assert 0 < int(mask.sum()) < h * w
    if kind == "atmax":
        assert int(mask.sum()) == 0
    # in place
    y = dx.clone()
    ops.p2p_local_blend(dmaps, S, R.BLEND_NK, sets, thr, y, out=y)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().view(torch.int32), gi), "the in-place launch differs"


def test_local_blend_refuses_three_samples(ops):
    maps = [torch.zeros(3, 256, 77, device=DEV)]
    x = torch.zeros(3, 4, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="exactly two samples"):
        ops.p2p_local_blend(maps, 16, 77, [[1], [1]], 0.3, x)
    with pytest.raises(ValueError, match="exactly two samples"):
        ops.p2p_local_blend([maps[0][:2].contiguous()], 16, 77, [[1], [1]], 0.3, x)


# ------------------------------------------------------------------------------------------------------------------ module level
UNET_P2P = dict(image_size=32, in_channels=4, model_channels=64, out_channels=4, num_res_blocks=2, attention_resolutions=[1, 2], channel_mult=[1, 2],
                num_head_channels=64, use_spatial_transformer=True, transformer_depth=1, context_dim=16, legacy=False, use_checkpoint=False)
PROMPTS = ["a cat sits on the grass", "a dog sits on the grass"]


def _ctx(prompts):
    """a seeded stand-in for the text encoder: 77 tokens of 16 channels per prompt"""
    out = []
    for p in prompts:
        gen = torch.Generator().manual_seed(1 + sum(ord(ch) * (i + 1) for i, ch in enumerate(p)) % 100003)
        out.append(torch.randn(77, 16, generator=gen))
    return torch.stack(out).to(DEV)


@pytest.fixture(scope="module")
def p2p_ldm():
    """the small UNet of util_models.py at head dim 64 on 32 x 32 latents with SD's store layout in small: two transformer blocks per level going
    down (1024, 1024, 256, 256 tokens), one in the middle (256), three per level going up (256 x 3, 1024 x 3): 22 CrossAttention modules, so that
    down_cross[2:4] + up_cross[:3] are the 16 x 16 maps LocalBlend reads"""
    from util_models import G, unzero, randomize_norm_affine
    from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from anyedit_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    torch.manual_seed(52)
    g = G(52)
    unet = UNetModel(**UNET_P2P)
    unzero(unet, g, std=0.05)
    randomize_norm_affine(unet, g)
    ldm = LatentDiffusion(unet.eval(), conditioning_key="crossattn", timesteps=1000, linear_start=0.00085, linear_end=0.0120).to(DEV)
    ldm.get_learned_conditioning = _ctx
    return ldm


def _eval_once(ldm):
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(1, 4, 32, 32, generator=gen).expand(4, -1, -1, -1).contiguous().to(DEV)
    t = torch.full((4,), 500, device=DEV, dtype=torch.long)
    ctx = torch.cat([_ctx([""] * 2), _ctx(PROMPTS)])
    with torch.no_grad():
        return ldm.apply_model(x, t, ctx).float().cpu()


def test_empty_control_and_store_leave_the_unet_bit_identical(p2p_ldm, RC):
    """EmptyControl and AttentionStore registered: the UNet output is bit-identical to the unregistered model's; the store equals the float64 head
    sums of the operands each call was handed, under the store bound; unregister restores the original launches."""
    import anyedit_amd.prompt2prompt as PP
    from anyedit_amd.ldm.modules.attention import CrossAttention
    plain = _eval_once(p2p_ldm)
    PP.register_attention_control(p2p_ldm, PP.EmptyControl())
    assert torch.equal(_eval_once(p2p_ldm), plain), "EmptyControl changed the output"
    assert PP.unregister(p2p_ldm) == 22

    class Rec(PP.AttentionStore):
        def forward(self, attn, is_cross, place, B, N, core, **operands):
            if is_cross:
                self.rec.append((place, attn.heads, attn.dim_head, attn.scale, N, operands["Nk"], operands["q"].cpu(), operands["kv"].cpu()))
            return super().forward(attn, is_cross, place, B, N, core, **operands)

    ctl = Rec()
    ctl.rec = []
    PP.register_attention_control(p2p_ldm, ctl)
    assert ctl.num_att_layers == 22
    assert torch.equal(_eval_once(p2p_ldm), plain), "AttentionStore changed the output"
    assert (ctl.cur_step, ctl.cur_att_layer) == (1, 0) and len(ctl.rec) == 11
    pos = {}
    for place, H, D, scale, N, Nk, q, kv in ctl.rec:
        i = pos.get(place, 0)
        pos[place] = i + 1
        inner = H * D
        Q = q.as_strided((4, H, N, D), (N * inner, D, inner, 1), 0).to(F64)
        K = kv.as_strided((4, H, Nk, D), (Nk * 2 * inner, D, 2 * inner, 1), 0).to(F64)
        _, Pp, W = R.p2p_ref(Q, K, None, scale, list(range(4)))
        got = ctl.attention_store[f"{place}_cross"][i].cpu()
        assert ctl.store_heads[f"{place}_cross"][i] == H and tuple(got.shape) == (2, N, Nk)
        bnd = R.p2p_store_bound(W, Nk, D, R.qk_abs(Q, K, scale), H)[2:]
        ratio = RC.bound_check(got.reshape(-1, Nk), Pp.sum(1)[2:].reshape(-1, Nk), bnd.reshape(-1, Nk), f"store {place}_cross[{i}]")
        print(f"store {place}_cross[{i}] N={N} H={H}: worst err/bound {ratio:.3f}")
    assert [len(ctl.attention_store[k]) for k in ("down_cross", "mid_cross", "up_cross")] == [4, 1, 6]
    assert PP.unregister(p2p_ldm) == 22
    assert not any("editor" in m.__dict__ for m in p2p_ldm.modules() if isinstance(m, CrossAttention))
    assert torch.equal(_eval_once(p2p_ldm), plain), "after unregister the output must be bit-identical to a model that never had a controller"


def _f64_replace(PP):
    class F64Replace(PP.AttentionReplace):
        """the same decisions, the edited samples of a live cross-attention carried out by the float64 statement on the device operands"""

        def _edited_cross(self, attn, place, B, N, q, kv, Nk, M, c, d):
            P, h, dh = B // 2, attn.heads, attn.dim_head
            inner = h * dh
            Q = q.as_strided((B, h, N, dh), (N * inner, dh, inner, 1), 0).to(F64)
            K = kv.as_strided((B, h, Nk, dh), (Nk * 2 * inner, dh, 2 * inner, 1), 0).to(F64)
            V = kv.as_strided((B, h, Nk, dh), (Nk * 2 * inner, dh, 2 * inner, 1), inner).to(F64)
            pad = lambda t, fill: torch.cat([torch.full_like(t, fill), t])     # the tables cover the conditional half: lay them over the batch
            r, Pp, _ = R.p2p_ref(Q, K, V, attn.scale, list(range(P)) + [P] * P, pad(M, 0.0), pad(c, 0.0), pad(d, 1.0))
            if N <= 32 ** 2:
                buf, acc = self._entry(place, P, N, Nk, h, q.device)
                s = Pp[P:].sum(1).float()
                buf.copy_(buf + s if acc else s)
            out = torch.empty(B, N, inner, dtype=q.dtype, device=q.device)
            want = r.permute(0, 2, 1, 3).reshape(B, N, inner)[P + 1:]
            out[P + 1:] = want.to(q.dtype)
            # the kernel on the SAME operands, for the per-call figures of the test
            kv2 = kv[P * Nk:]
            qs, ks = (N * inner, dh, inner), (Nk * 2 * inner, dh, 2 * inner)
            from anyedit_amd import ops
            k_out = ops.attention_p2p(q[P * N:], kv2, kv2[:, inner:], P, h, N, Nk, dh, attn.scale, qs, ks, ks, [0] * P, M=M, c=c, d=d)[1:].to(F64)
            self.per_call.append((float((k_out - want).norm() / want.norm()), float((k_out - want).abs().max() / want.abs().max())))
            # the unconditional half and the base are not edited: the launch the controller itself issues for them
            ops.attention(q, kv, kv[:, inner:], P + 1, h, N, Nk, dh, attn.scale, qs, ks, ks, out=out[:P + 1])
            return out
    return F64Replace


def _first_order_gain(ldm, n):
    """sum over the n uniform DDIM steps of |d x_prev / d eps| = |sqrt(1 - a_prev) - sqrt(a_prev) sqrt(1 - a_t) / sqrt(a_t)|: what a perturbation of
    the network's output is multiplied by on its way into the latents, per unit of guidance scale, to first order"""
    ac = ldm.alphas_cumprod.double().cpu()
    ts = [i * (1000 // n) + 1 for i in range(n)]
    g = 0.0
    for i in range(n):
        a, ap = float(ac[ts[i]]), float(ac[ts[i - 1]] if i else ac[0])
        g += abs((1 - ap) ** 0.5 - ap ** 0.5 * (1 - a) ** 0.5 / a ** 0.5)
    return g


def _guidance(ldm):
    """The latents tolerance borrowed from MasaCtrl's end-to-end test (tests/test_hip_unet.py's `close`) belongs to a TWO-step run at guidance scale
    7.5.  A rounding-level difference d in the conditional branch's eps enters the latents as scale x gain x d; the first-order gain of the four
    steps used here is 2.73 against 1.59 for two steps (this schedule), so the run takes the scale at which the two products agree: 7.5 x 1.59 /
    2.73 = 4.37.  (At 7.5 the four-step run measured rel_l2 2.5e-2 and 49.5 dB with per-call outputs that agree to a bf16 ulp: the difference
    is the sampler's amplification, not the kernel's.)"""
    return 7.5 * _first_order_gain(ldm, 2) / _first_order_gain(ldm, 4)


def _run(ldm, ctl, steps=4):
    import anyedit_amd.prompt2prompt as PP
    from anyedit_amd.ldm.models.diffusion.ddim import DDIMSampler
    gen = torch.Generator().manual_seed(21)
    latent = torch.randn(1, 4, 32, 32, generator=gen).to(DEV)
    out, start = PP.text2image_ldm_stable(ldm, DDIMSampler(ldm), PROMPTS, ctl, num_inference_steps=steps, guidance_scale=_guidance(ldm), latent=latent,
                                          decode=False)
    assert start is latent
    return out.float().cpu()


def test_attention_replace_on_the_unet(p2p_ldm):
    """AttentionReplace over 4 steps, crossing both gates (the default cross gate and the self gate close after step 1; the key word's stays open):
    the calls taken over are those the protocol's constants give; the edited rows of every live call agree with the float64 statement on the same
    operands under the forward output's tolerance of MasaCtrl's end-to-end test (relative L2 6e-3, max-abs over max 3e-2); and the latents match the
    same controller driven by the float64 statement under its latents tolerance, tests/test_hip_unet.py's `close` (relative L2 2e-2, 38 dB), at the
    guidance scale `_guidance` derives for four steps."""
    import anyedit_amd.prompt2prompt as PP
    from conftest import rel_l2, psnr
    tok = R.ToyTokenizer()
    args = (PROMPTS, 4, R.cross_steps("dog"), 0.5)
    log = []

    class Logged(PP.AttentionReplace):
        def forward(self, attn, is_cross, place, B, N, core, **operands):
            log.append((self.cur_step, self.cur_att_layer, is_cross, N))
            return super().forward(attn, is_cross, place, B, N, core, **operands)

    ctl = Logged(*args, tokenizer=tok)
    got = _run(p2p_ldm, ctl)
    assert (ctl.cur_step, ctl.cur_att_layer) == (4, 0) and len(log) == 4 * 22
    expect = [(s, l, "cross" if x else "self") for s, l, x, N in log if x or (s < 2 and N <= 256)]
    assert ctl.controlled == expect
    assert sum(k == "self" for _, _, k in expect) == 2 * 6 and sum(k == "cross" for _, _, k in expect) == 4 * 11
    ref_ctl = _f64_replace(PP)(*args, tokenizer=tok)
    ref_ctl.per_call = []
    want = _run(p2p_ldm, ref_ctl)
    assert ref_ctl.controlled == expect
    worst = (max(a for a, _ in ref_ctl.per_call), max(b for _, b in ref_ctl.per_call))
    print(f"AttentionReplace: guidance scale {_guidance(p2p_ldm):.3f}; edited rows of {len(ref_ctl.per_call)} live calls, kernel against float64 on the same "
          f"operands: worst rel_l2 {worst[0]:.3e} (<= 6e-3), max_abs/max {worst[1]:.3e} (<= 3e-2)")
    assert len(ref_ctl.per_call) == 4 * 11 and worst[0] <= 6e-3 and worst[1] <= 3e-2
    plain = _run(p2p_ldm, PP.EmptyControl())
    e, p = rel_l2(got, want), psnr(got, want)
    print(f"AttentionReplace: latents rel_l2 {e:.3e} (<= 2e-2), psnr {p:.1f} dB (>= 38); against the unedited pair rel_l2 {rel_l2(got, plain):.3e}")
    assert e <= 2e-2 and p >= 38.0
    assert torch.equal(got[0], plain[0]), "prompt 0 (the base) must keep the bits of a run without a controller"
    assert not torch.equal(got[1], plain[1]), "the controller changed nothing on the edited prompt"


def test_text2image_with_local_blend(p2p_ldm):
    """text2image_ldm_stable with AttentionReplace + LocalBlend runs, returns the base image unchanged for prompt 0, and leaves no editor behind"""
    import anyedit_amd.prompt2prompt as PP
    from anyedit_amd.ldm.modules.attention import CrossAttention
    tok = R.ToyTokenizer()
    calls = []

    class Watched(PP.LocalBlend):
        def __call__(self, x_t, store):
            out = super().__call__(x_t, store)
            calls.append(float((out[1] != x_t[1]).float().mean()))
            assert torch.equal(out[0], x_t[0])
            return out

    lb = Watched(PROMPTS, ("cat", "dog"), threshold=0.3, tokenizer=tok)
    ctl = PP.AttentionReplace(PROMPTS, 4, R.cross_steps("dog"), 0.5, local_blend=lb, tokenizer=tok)
    got = _run(p2p_ldm, ctl)
    plain = _run(p2p_ldm, PP.EmptyControl())
    print(f"LocalBlend: fraction of the edited latent taken from the base per step {calls}")
    assert len(calls) == 4 and torch.isfinite(got).all()
    assert torch.equal(got[0], plain[0]), "prompt 0 must come back unchanged"
    assert not any("editor" in m.__dict__ for m in p2p_ldm.modules() if isinstance(m, CrossAttention))
