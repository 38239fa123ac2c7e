"""tests/rowpanel_ref.py without a GPU: its references and bounds must accept an fp32 emulation of every route of gemm_rowpanel.hip /
ff_fused.hip and reject each of fourteen wrong kernels.

The emulation follows the kernels' structure in fp32 torch — 192-row panels whose rows >= M read as zeros, 32-column chunks in pairs, the
image-row order rp_wrow, GEGLU's halved `a` bias, the LayerNorm prologue rounded to bf16, the fold from five statistics slices, the row
statistics parked per half and pair, the W2 image read back with its piece rotation — and writes into sentinel-filled buffers with guard
rows.  Each fault changes one of those places:
  wrow          two 4-column groups of rp_wrow swapped                       bias_gate     GEGLU bias halved on the gate instead of `a`
  swap          `a` and gate swapped                                         res_chunk     residual taken from the neighbouring 32-column chunk
  rs_slice      the last pair's row statistics written to slice npairs - 2   rs_halves     the two halves' statistics not added
  fold_slice    fold slice 4 of 5 dropped                                    fold_row      fold with the statistics of the next row
  eps           LayerNorm eps outside the root                               rotation      W2 image read without the piece rotation
  chunk         one 16-unit hidden chunk skipped                             b2            b2 missing
  r3            residual3 missing                                            row           a row >= M stored (seen by the guards)
Also here: the ambiguous share of every LayerNorm-prologue case (<= 10 %, from the reference alone) and the shape of the case list / ledger."""
import pytest
import torch

import route_cases as RC
import rowpanel_ref as RR

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
K, EPS = RR.K, 1e-5
GUARD = 8
BF_SENT = 0x7FA5
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from anyedit_amd import ops as o      # host-side packing only: pack_geglu, pack_ff2_fused
    return o


# --------------------------------------------------------------------------------------------------- emulation
def _buf(M, n):
    b = torch.empty(M + GUARD, n, dtype=BF)
    b.view(torch.int16).fill_(BF_SENT)
    return b


def _guards_ok(b, M):
    return bool((b.view(torch.int16)[M:] == BF_SENT).all())


def _wrow(i, fault):
    if fault == "wrow":      # image rows 4..7 <-> 20..23: W rows 8..11 and 12..15 change places
        i = torch.where((i >= 4) & (i < 8), i + 16, torch.where((i >= 20) & (i < 24), i - 16, i))
    return 8 * ((i & 15) >> 2) + 4 * (i >> 4) + (i & 3)


def emulate(A, W, bias=None, res=None, geglu=False, ln=None, fold=None, rs=False, fault=""):
    """A [M, K] bf16, W [N, K] bf16 in the kernel's layout (ops.pack_geglu for GEGLU).  ln = (gamma, beta, eps): prologue;
    fold = (stats [M, 5, 2], s, eps): `bias` then holds c.  -> (guarded output [M + GUARD, n_out], row statistics [M, N / 64, 2] or None)"""
    M, N = A.shape[0], W.shape[0]
    Mp = (M + 191) // 192 * 192
    x = torch.zeros(Mp, K)
    x[:M] = A.float()
    if ln:
        gamma, beta, eps = ln
        mu = x.mean(1, keepdim=True)
        v = ((x - mu) ** 2).mean(1, keepdim=True)
        rstd = 1.0 / (v.sqrt() + eps) if fault == "eps" else (v + eps).rsqrt()
        x = ((x - mu) * rstd * gamma + beta).to(BF).float()
    Wf = W.float()
    n_out = N // 2 if geglu else N
    out = _buf(M, n_out)
    rows = torch.arange(Mp)
    rok = rows < (M + 1 if fault == "row" else M)
    rcl = rows.clamp(max=M - 1)
    sb = bias.float().clone() if bias is not None else torch.zeros(N)
    if geglu:
        halved = ((torch.arange(N) & 16) == 0) != (fault == "bias_gate")
        sb = torch.where(halved, 0.5 * sb, sb)
    if fold:
        stats, s, eps = fold
        st = stats[(rows + 1).clamp(max=M - 1) if fault == "fold_row" else rcl]
        parts = st.shape[1] - (1 if fault == "fold_slice" else 0)
        sm, sq = st[:, :parts, 0].sum(1, keepdim=True), st[:, :parts, 1].sum(1, keepdim=True)
        mu = sm / K
        r = ((sq / K - mu * mu).clamp(min=0) + eps).rsqrt()
        t = -r * mu
    npairs = N // 64
    stat = torch.full((M + GUARD, npairs, 2), NAN) if rs else None
    i = torch.arange(32)
    parked = {}
    for c in range(N // 32):
        n0, pi, half = 32 * c, c // 2, c % 2
        acc = x @ Wf[n0 + (i if geglu else _wrow(i, fault))].t()        # [Mp, 32] in image-row order
        if geglu:
            aa, gg = acc[:, :16], acc[:, 16:]
            ba, bg = sb[n0:n0 + 16], sb[n0 + 16:n0 + 32]
            if fold:
                ah, g = aa * (0.5 * r) + ((0.5 * t) * s[n0:n0 + 16] + ba), gg * r + (t * s[n0 + 16:n0 + 32] + bg)
            else:
                ah, g = 0.5 * aa + ba, gg + bg
            if fault == "swap":
                ah, g = 0.5 * g, 2.0 * ah
            o = ah * (g + g * torch.erf(g * 0.5 ** 0.5))
            out[rok.nonzero()[:, 0], n0 // 2:n0 // 2 + 16] = o[rok].to(BF)
        else:
            o = torch.empty(Mp, 32)
            o[:, 8 * ((i & 15) >> 2) + 4 * (i >> 4) + (i & 3)] = acc       # a lane's two fragments are eight consecutive columns
            o = o * r + (t * s[n0:n0 + 32] + sb[n0:n0 + 32]) if fold else o + sb[n0:n0 + 32]
            if res is not None:
                rn = n0 ^ 32 if fault == "res_chunk" else n0
                o = o + res[rcl, rn:rn + 32].float()
            pk = o.to(BF)
            out[rok.nonzero()[:, 0], n0:n0 + 32] = pk[rok]
            if rs:
                pf = pk.float()
                parked[half] = torch.stack([pf.sum(1), (pf * pf).sum(1)], -1)
                if half == 1:
                    tot = parked[0] if fault == "rs_halves" else parked[0] + parked[1]
                    sl = pi - 1 if (fault == "rs_slice" and pi == npairs - 1) else pi
                    stat[rok.nonzero()[:, 0], sl] = tot[rok]
    return out, stat


def w2_from_image(img, rotation=True):
    """the [C, H] weight the kernel multiplies when lane group g reads 16-byte piece (g + 2 ((i & 15) >> 2)) & 3 of image row i"""
    S, C, _ = img.shape
    w = torch.zeros(C, 32 * S)
    i = torch.arange(C)
    col = 32 * (i >> 5) + 8 * ((i & 15) >> 2) + 4 * ((i & 31) >> 4) + (i & 3)
    e = torch.arange(8)
    for g in range(4):
        pos = (g + 2 * ((i & 15) >> 2)) & 3 if rotation else torch.full_like(i, g)
        piece = torch.gather(img.float(), 2, (8 * pos[None, :, None] + e[None, None, :]).expand(S, C, 8))      # [S, C, 8]
        unit = 16 * (e >> 2) + 4 * g + (e & 3)
        for s in range(S):
            w[col[:, None], (32 * s + unit)[None, :]] = piece[s]
    return w


def emulate_ff(ops, x, gamma, beta, w1p, b1p, w2img, b2, res, proj=None, fault=""):
    """-> (h_s [M, H] bf16, guarded y or z)"""
    M, H = x.shape[0], w1p.shape[0] // 2
    h = emulate(x, w1p, b1p, geglu=True, ln=(gamma, beta, EPS))[0][:M]
    hf = h.float()
    if fault == "chunk":
        hf[:, 48:64] = 0.0
    y = hf @ w2_from_image(w2img, fault != "rotation").t() + (0.0 if fault == "b2" else b2)
    if res is not None:
        y = y + res.float()
    out = _buf(M, K)
    if proj is None:
        out[:M] = y.to(BF)
        return h, out
    w3, b3, r3 = proj
    z = y.to(BF).float() @ w3.float().t() + (b3 if b3 is not None else 0.0)
    if r3 is not None and fault != "r3":
        z = z + r3.float()
    out[:M] = z.to(BF)
    return h, out


# --------------------------------------------------------------------------------------------------- operands
def _operands(M, N, geglu, ops, seed=3):
    gen = torch.Generator().manual_seed(seed)
    x = RR.make_rows(gen, M)
    w = RR.make_weight(gen, N, K).to(BF)
    b = RR.make_bias(gen, N)
    gamma, beta = RR.make_affine(gen)
    res = torch.randn(M, N, generator=gen).to(BF)
    wk, bk = ops.pack_geglu(w, b) if geglu else (w, b)
    return x, w, b, gamma, beta, res, wk, bk


def _accepts(out, M, ref, bnd):
    assert _guards_ok(out, M)
    return RR.check(out[:M], ref, bnd, "output") <= 1.0


def _rejects(out, M, ref, bnd):
    if not _guards_ok(out, M):
        return True
    with pytest.raises(RR.CaseFailure):
        RR.check(out[:M], ref, bnd, "output")
    return True


# --------------------------------------------------------------------------------------------------- tests
def test_bf16_grid_in_float64():
    v = torch.randn(4096, dtype=F64) * torch.logspace(-6, 3, 4096, dtype=F64)
    assert torch.equal(RR.round_bf16(v.float().to(F64)), v.float().to(BF).to(F64))          # fp32 -> bf16 is one rounding in torch too
    assert torch.equal(RR.round_bf16(torch.tensor([1.00390625, 1.01171875], dtype=F64)), torch.tensor([1.0, 1.015625], dtype=F64))   # ties to even
    assert torch.equal(RR.ulp_bf16(torch.tensor([1.0, 1.99, 0.75, -3.0], dtype=F64)), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6], dtype=F64))


@pytest.mark.parametrize("M,N", [(193, 128), (241, 320)])
def test_plain_routes_are_accepted_and_every_fault_rejected(ops, M, N):
    x, w, b, _, _, res, _, _ = _operands(M, N, False, ops)
    ref, bnd = RR.gemm_ref(x, w, b, res)
    assert _accepts(emulate(x, w, b, res)[0], M, ref, bnd)
    for fault in ("wrow", "res_chunk", "row"):
        assert _rejects(emulate(x, w, b, res, fault=fault)[0], M, ref, bnd), fault
    # GEGLU on the chunk(2) semantics through ops.pack_geglu
    x, w, b, _, _, _, wk, bk = _operands(M, N, True, ops)
    ref, bnd = RR.gemm_ref(x, w, b, None, geglu=True)
    assert _accepts(emulate(x, wk, bk, geglu=True)[0], M, ref, bnd)
    for fault in ("bias_gate", "swap", "row"):
        assert _rejects(emulate(x, wk, bk, geglu=True, fault=fault)[0], M, ref, bnd), fault
    # the un-packed weight in the packed kernel: the packing itself is under test
    assert _rejects(emulate(x, w, b, geglu=True)[0], M, ref, bnd)


@pytest.mark.parametrize("N", [128, 320])
def test_row_statistics_are_accepted_and_both_faults_rejected(ops, N):
    M = 209
    x, w, b, _, _, res, _, _ = _operands(M, N, False, ops, seed=4)
    out, st = emulate(x, w, b, res, rs=True)
    assert torch.equal(out.view(torch.int16), emulate(x, w, b, res)[0].view(torch.int16))
    assert (st[M:] != st[M:]).all(), "statistics rows past M stay untouched"
    assert RR.row_stats_check(st[:M], out[:M]) <= 1.0
    for fault in ("rs_slice", "rs_halves"):
        _, bad = emulate(x, w, b, res, rs=True, fault=fault)
        with pytest.raises(RR.CaseFailure):
            RR.row_stats_check(bad[:M], out[:M])


@pytest.mark.parametrize("geglu,N", [(False, 192), (True, 128)])
def test_fold_is_accepted_and_both_faults_rejected(ops, geglu, N):
    M = 207
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=gen).to(BF)
    wp, bp, r = RR.make_weight(gen, K, K).to(BF), RR.make_bias(gen, K), RR.make_rows(gen, M, K)
    xs, st = emulate(a, wp, bp, r, rs=True)
    xs, st = xs[:M], st[:M]
    w, b = RR.make_weight(gen, N, K), RR.make_bias(gen, N)
    gamma, beta = RR.make_affine(gen)
    res = None if geglu else torch.randn(M, N, generator=gen).to(BF)
    wq, s, c = RR.pack_ln_fold_ref(w, b, gamma, beta, geglu, ops.pack_geglu)
    ref, bnd = RR.fold_ref(xs, wq, s, c, EPS, res, geglu)
    # the fold computes what LayerNorm + Linear compute (float64, un-rounded weights): within the rounding of W' alone
    z = torch.nn.functional.layer_norm(xs.to(F64), (K,), gamma.to(F64), beta.to(F64), EPS) @ w.to(F64).t() + b.to(F64)
    want = z.chunk(2, 1)[0] * RR.gelu64(z.chunk(2, 1)[1]) if geglu else z + res.to(F64)
    assert float((ref - want).abs().max()) <= 2e-2 * float(want.abs().max())
    assert _accepts(emulate(xs, wq, c, res, geglu=geglu, fold=(st, s, EPS))[0], M, ref, bnd)
    for fault in ("fold_slice", "fold_row", "wrow" if not geglu else "bias_gate"):
        assert _rejects(emulate(xs, wq, c, res, geglu=geglu, fold=(st, s, EPS), fault=fault)[0], M, ref, bnd), fault


@pytest.mark.parametrize("geglu,N", [(False, 192), (True, 256)])
def test_prologue_is_accepted_and_every_fault_rejected(ops, geglu, N):
    M = 239
    x, w, b, gamma, beta, res, wk, bk = _operands(M, N, geglu, ops, seed=6)
    res = None if geglu else res
    ref, bnd, share = RR.ln_gemm_ref(x, gamma, beta, EPS, w, b, res, geglu)
    assert 0.0 < share <= RR.AMBIGUOUS_CAP
    assert _accepts(emulate(x, wk, bk, res, geglu=geglu, ln=(gamma, beta, EPS))[0], M, ref, bnd)
    for fault in ("eps", "row", "swap" if geglu else "wrow"):
        assert _rejects(emulate(x, wk, bk, res, geglu=geglu, ln=(gamma, beta, EPS), fault=fault)[0], M, ref, bnd), fault
    # ONE wrong k term (a typical operand, |z| about 1, left out of one row): several times the bound on most of the row's outputs
    p = RR.ln_prologue(x, gamma, beta, EPS)
    row = 5
    k = int((p["zb"][row].abs() - 1.0).abs().argmin())
    zb = p["zb"].clone()
    zb[row, k] = 0.0
    pre = zb @ w.to(F64).t() + b.to(F64)
    bad = (pre.chunk(2, 1)[0] * RR.gelu64(pre.chunk(2, 1)[1]) if geglu else pre + res.to(F64))
    over = ((bad - ref).abs() / bnd)[row]
    print(f"one k term left out: error / bound median {float(over.median()):.1f}, max {float(over.max()):.1f}; bound / output rounding median "
          f"{float((bnd / (2.0 ** -8 * ref.abs() + 1e-30)).median()):.2f}")
    assert float(over.median()) > 1.0 and float(over.max()) > 4.0


@pytest.mark.parametrize("H", [64, 128])
def test_feed_forward_is_accepted_and_every_fault_rejected(ops, H):
    M = 193
    gen = torch.Generator().manual_seed(7 + H)
    x = RR.make_rows(gen, M)
    w1, b1 = RR.make_weight(gen, 2 * H, K).to(BF), RR.make_bias(gen, 2 * H)
    w2, b2 = RR.make_weight(gen, K, H), RR.make_bias(gen, K)
    gamma, beta = RR.make_affine(gen)
    res = torch.randn(M, K, generator=gen).to(BF)
    w3, b3, r3 = RR.make_weight(gen, K, K).to(BF), RR.make_bias(gen, K), torch.randn(M, K, generator=gen).to(BF)
    w1p, b1p = ops.pack_geglu(w1, b1)
    img = ops.pack_ff2_fused(w2)
    assert torch.equal(w2_from_image(img), w2.to(BF).float()), "the image read back with its rotation is W2"
    h_s, y = emulate_ff(ops, x, gamma, beta, w1p, b1p, img, b2, res)
    ref, bnd, share = RR.ln_gemm_ref(x, gamma, beta, EPS, w1, b1, None, True)
    assert share <= RR.AMBIGUOUS_CAP and RR.check(h_s, ref, bnd, "hidden") <= 1.0
    dev = RR.hidden_deviation(ref, bnd)
    print(f"H = {H}: {float((dev > 0).to(F64).mean()):.3f} of the hidden values may be stored differently by two correct kernels")
    ref, bnd = RR.gemm_ref(h_s, w2.to(BF), b2, res)                 # the hidden activation the emulated kernel itself used: the tight rule
    ref_w, bnd_w = RR.gemm_ref(h_s, w2.to(BF), b2, res, dev=dev)    # as if h_s came from another correct kernel: the widened rule
    assert _accepts(y, M, ref, bnd) and _accepts(y, M, ref_w, bnd_w)
    for fault in ("rotation", "chunk", "b2"):
        bad = emulate_ff(ops, x, gamma, beta, w1p, b1p, img, b2, res, fault=fault)[1]
        assert _rejects(bad, M, ref, bnd) and _rejects(bad, M, ref_w, bnd_w), fault
    # a hidden activation from a kernel whose prologue rounded ONE operand of a row to its other neighbour (what the two kernels do to each other on
    # the GPU): outside the tight rule for some seed, always inside the widened one
    p = RR.ln_prologue(x, gamma, beta, EPS)
    row = 7
    k = int((p["dev"][row] > 0).nonzero()[0])
    zb = p["zb"].clone()
    zb[row, k] += p["dev"][row, k] * (1.0 if RR.round_bf16(p["z"] + p["al"])[row, k] > zb[row, k] else -1.0)
    pre = zb[row:row + 1] @ w1.to(F64).t() + b1.to(F64)
    h_other = h_s.clone()
    h_other[row] = (pre.chunk(2, 1)[0] * RR.gelu64(pre.chunk(2, 1)[1])).to(BF)[0]
    assert int((h_other.view(torch.int16) != h_s.view(torch.int16)).sum()) > 0
    ref_o, bnd_o = RR.gemm_ref(h_other, w2.to(BF), b2, res, dev=dev)
    assert _accepts(y, M, ref_o, bnd_o)
    # projection: against the stored feed-forward output of the same operands
    y_s = y[:M]
    for b3_, r3_ in ((b3, r3), (None, r3), (b3, None)):
        ref, bnd = RR.gemm_ref(y_s, w3, b3_, r3_)
        assert _accepts(emulate_ff(ops, x, gamma, beta, w1p, b1p, img, b2, res, proj=(w3, b3_, r3_))[1], M, ref, bnd)
    ref, bnd = RR.gemm_ref(y_s, w3, b3, r3)
    assert _rejects(emulate_ff(ops, x, gamma, beta, w1p, b1p, img, b2, res, proj=(w3, b3, r3), fault="r3")[1], M, ref, bnd)
    assert _rejects(emulate_ff(ops, x, gamma, beta, w1p, b1p, img, b2, res, proj=(w3, b3, r3), fault="chunk")[1], M, ref, bnd)


def _prologue_operands(c):
    """the (x, gamma, beta) tools/rowpanel_route_check.py draws for a case: same generator, same order"""
    import zlib
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = RR.make_rows(gen, c["M"])
    if c["op"] == "rp":
        RR.make_weight(gen, c["N"], K)
        if c.get("bias", True):
            RR.make_bias(gen, c["N"])
    else:
        H = c["H"]
        RR.make_weight(gen, 2 * H, K), RR.make_bias(gen, 2 * H), RR.make_weight(gen, K, H), RR.make_bias(gen, K)
    return (x,) + RR.make_affine(gen)


@pytest.mark.parametrize("cid", [c["id"] for c in RC.ROWPANEL_CASES if c["op"] == "ff" or c.get("lnm") == 1])
def test_ambiguous_share_of_every_prologue_case(cid):
    c = next(c for c in RC.ROWPANEL_CASES if c["id"] == cid)
    x, gamma, beta = _prologue_operands(c)
    share = RR.ln_prologue(x, gamma, beta, EPS)["share"]
    print(f"{cid}: ambiguous share {share:.4f}")
    assert share <= RR.AMBIGUOUS_CAP


def test_rowpanel_cases_and_ledger_are_well_formed():
    ids = RC.ROWPANEL_CASE_IDS
    assert len(set(ids)) == len(ids) and not set(ids) & (set(RC.CASE_IDS) | set(RC.NORM_CASE_IDS)), "duplicate case ids"
    assert not set(RC.ROWPANEL_LEDGER) & (set(RC.LEDGER) | set(RC.NORM_LEDGER))
    byid = {c["id"]: c for c in RC.ROWPANEL_CASES}
    for key, (kind, what) in RC.ROWPANEL_LEDGER.items():
        assert kind == "default" and what and all(i in byid for i in what), key
        ms = [byid[i]["M"] for i in what]
        assert any(m % 16 for m in ms) and any(m % 192 == 0 for m in ms), f"{key}: needs a ragged M and a whole number of blocks, has {ms}"
    listed = {i for _, what in RC.ROWPANEL_LEDGER.values() for i in what}
    tiled = {c["id"] for c in RC.ROWPANEL_CASES if c.get("tiled")}
    assert set(ids) - listed == tiled and len(tiled) == 2, "every case asserts a route; the two below the threshold assert the tiled kernel"
    for c in RC.ROWPANEL_CASES:
        assert c["op"] in ("rp", "rs", "chain", "ff") and c["env"] in ("hook", "default") and c["M"] >= 192
        if c["op"] != "ff":
            assert c["N"] % 64 == 0 and c["N"] <= 2560
        assert (c["env"] == "default") == (c["M"] >= RC.RP_THRESHOLD_M - 1)
        assert bool(c.get("tiled")) == (c["M"] == RC.RP_THRESHOLD_M - 1)
    blocks = lambda m: (m + 191) // 192     # noqa: E731
    assert blocks(RC.RP_THRESHOLD_M) == 192 and blocks(RC.RP_THRESHOLD_M - 1) == 191
    # the pair-count edges, on every kind of launch that has them
    npairs = lambda **kw: {c["N"] // 64 for c in RC.ROWPANEL_CASES if all(c.get(k) == v for k, v in kw.items())}     # noqa: E731
    assert npairs(op="rp", epi="none", lnm=0) >= {1, 2, 3, 4, 5, 15, 40}
    assert npairs(op="rp", epi="geglu", lnm=0) >= {2, 40} and npairs(op="rp", epi="geglu", lnm=1) >= {2, 40}
    assert npairs(op="rs") >= {1, 2, 5}
    assert npairs(op="chain", epi="none") >= {15} and npairs(op="chain", epi="geglu") >= {40}
    ff = [c for c in RC.ROWPANEL_CASES if c["op"] == "ff"]
    assert {c["H"] for c in ff} >= {64, 128, 1280} and {c["M"] for c in ff if c["env"] == "hook"} >= {192, 193, 241, 383}
    assert any(c["strided"] for c in ff) and {c["res"] for c in ff} == {True, False}
    for k in ("b3", "r3", "cs"):
        assert {c["proj"][k] for c in ff if c["proj"]} == {True, False}, k
